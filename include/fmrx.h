/* include/fmrx.h — C ABI of the MI355X-native FM receive chain (libfmrx.so).
 *
 * Drop-in boundary for the per-block processing stage of the reference
 * (mehtas30/Software-Defined-Radio-Course-Project).  Plain C types only: pointers, sizes,
 * ints.  Every entry point returns an int status (FMRX_OK == 0, < 0 on error) instead of
 * calling exit() like the reference does.
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   fmrx_impulse_response_lpf  <- impulseResponseLPF   include/filter.h:15, src/filter.cpp:14-37
 *   fmrx_impulse_response_bpf  <- impulseResponseBPF   include/filter.h:17, src/filter.cpp:39-64
 *   fmrx_resample              <- resample             include/filter.h:19, src/filter.cpp:67-103
 *   fmrx_fm_demod              <- FMDemod              include/filter.h:21, src/filter.cpp:106-133
 *   fmrx_pll                   <- PLL                  include/filter.h:23, src/filter.cpp:136-174
 *   fmrx_mixer                 <- mixer                include/filter.h:25, src/filter.cpp:176-184
 *   fmrx_lr_extraction         <- LRExtraction         include/filter.h:27, src/filter.cpp:186-199
 *   fmrx_normalize_iq          <- readStdinBlockData   include/iofunc.h:28, src/iofunc.cpp:62-69
 *                                 + deinterleave       src/project.cpp:56-62
 *   fmrx_rf_block              <- rf_thread loop body  src/project.cpp:48-70
 *   fmrx_audio_block           <- audio_thread body    src/project.cpp:132-195
 *   fmrx_process               <- both bodies fused (host buffers in, host PCM out)
 *   fmrx_process_device        <- both bodies fused, device-resident buffers, async
 *   fmrx_rds_block_rec / _device   <- rds_thread body      src/project.cpp:200-271 (RDS front half;
 *                                 never launched by the reference, :380-382)
 *   fmrx_rds_bits / _device,      no counterpart: the RDS back half (symbol-rate resampler, bits,
 *   fmrx_rds_parse, _decode ...   block syndromes, group parser), defined below
 *   fmrx_set_deemphasis,          no counterpart: the reference never de-emphasises (its audio goes
 *   fmrx_deemph, _design          from the low-pass or LRExtraction straight into the quantiser)
 *   fmrx_fm_demod_arctan       <- fmDemodArctan        model/fmSupportLib.py:34-63
 *   fmrx_estimate_psd          <- estimatePSD          include/fourier.h:27-31, src/fourier.cpp:35-117
 *   fmrx_psd_device               (model/fmSupportLib.py:83-157)
 *
 * Buffers: functions named *_device / fmrx_resample etc. take DEVICE pointers and enqueue on
 * the context's HIP stream; fmrx_rf_block / fmrx_audio_block / fmrx_process take HOST
 * pointers and return when the result is in host memory.  The caller owns every buffer.
 */
#ifndef FMRX_H
#define FMRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMRX_OK 0
#define FMRX_EINVAL (-1)   /* bad argument / configuration */
#define FMRX_EHIP (-2)     /* HIP runtime error (no device, launch failure, ...) */
#define FMRX_ENOMEM (-3)   /* device or host allocation failed */
#define FMRX_ESTATE (-4)   /* state blob size/version mismatch */

/* Output semantics (SURVEY §7 hard part 3). */
#define FMRX_STEREO 2        /* project.cpp output: S16 interleaved R,L; shared audio_state  */
#define FMRX_MONO 1          /* mono S16 with a private audio history (project.cpp:146 with  */
                             /* its own state vector: fmMonoBlock-style receiver)            */

typedef struct {
    int mode;        /* 0..3, src/project.cpp:327-362                                         */
    int channels;    /* FMRX_MONO or FMRX_STEREO                                              */
    int rf_taps;     /* RF LPF taps, reference 51 (project.cpp:306); 0 = default              */
    int bp_taps;     /* stereo band-pass taps, reference 51 (project.cpp:307); 0 = default   */
    int audio_taps;  /* audio LPF taps per phase: 51 only (project.cpp:319; x up in 2/3)    */
    int n_streams;   /* independent IQ streams processed per call (>=1, <= the device's grid.y */
                     /* limit; fmrx_create refuses more with FMRX_EINVAL).  Device memory per   */
                     /* stream: 2 halos (~26 KiB) + the audio history; stereo adds the demod /  */
                     /* channel / carrier rows (3 x 4 B per IF sample of a call) and the PLL    */
                     /* scratch: ~32.5 B per sample of a segment (2^18 samples per stream, fewer */
                     /* past 32 streams: segment x streams ~2^23, >= 2^14 -- ~0.5 MB a stream at */
                     /* 2,048 streams) plus the call's trigArgs, 4 B per IF sample of a call (the */
                     /* NCO reads them after the runners; one 1 GiB mode-0 call: ~200 MB; the    */
                     /* pipelined engine from 16 streams holds two such side buffers).           */
    int device;      /* HIP device ordinal                                                     */
} fmrx_config;

typedef struct {
    int rf_fs, rf_decim, if_fs, bp_fs, audio_up, audio_down;
    int rf_taps, bp_taps, audio_taps_total; /* audio_taps_total = audio_taps * audio_up      */
    size_t block_bytes;   /* u8 per block, project.cpp:364 (256 * rf_decim * audio_decim)     */
    size_t iq_pairs;      /* block_bytes / 2                                                  */
    size_t if_samples;    /* demod floats per block                                           */
    size_t audio_frames;  /* audio frames per block                                           */
    size_t pcm_samples;   /* int16 per block = audio_frames * channels                        */
} fmrx_geometry_t;

typedef struct fmrx_ctx fmrx_ctx;

/* ---- configuration & lifetime ------------------------------------------------------- */
int fmrx_config_default(fmrx_config* cfg, int mode, int channels);
int fmrx_geometry(const fmrx_config* cfg, fmrx_geometry_t* geo);
int fmrx_create(const fmrx_config* cfg, fmrx_ctx** out);
void fmrx_destroy(fmrx_ctx* ctx);
int fmrx_reset(fmrx_ctx* ctx);                         /* back to the power-on state        */
const char* fmrx_last_error(void);                     /* thread-local message              */
const char* fmrx_version(void);

/* ---- stream state (checkpoint / resume) ---------------------------------------------- */
int fmrx_state_size(const fmrx_ctx* ctx, size_t* bytes);
int fmrx_get_state(fmrx_ctx* ctx, void* buf, size_t bytes);
int fmrx_set_state(fmrx_ctx* ctx, const void* buf, size_t bytes);

/* ---- time shards of one recording (mono product) ------------------------- */
/* The mono product has finite memory: the RF FIR (rf_taps - 1 I/Q pairs), the demodulator's
 * previous sample and the audio FIR depend only on a bounded run of raw bytes.  fmrx_seek
 * makes the NEXT call continue a stream whose bytes before it are `prev` (per stream, the n
 * bytes ending right before the call's first byte; stream-major, n_streams x n; n may be
 * anything -- fewer than fmrx_history_bytes means the stream began inside them), so a shard
 * of a recording that starts at a block boundary yields exactly the mono PCM the whole
 * recording yields there.  prev_on_device: 0 host pointer, 1 device pointer.  MONO contexts
 * only (the stereo PLL is a serial recurrence: FMRX_ESTATE); until the next fused call,
 * fmrx_audio_block has no valid history and returns FMRX_ESTATE.                        */
int fmrx_history_bytes(const fmrx_ctx* ctx, size_t* bytes);
int fmrx_seek(fmrx_ctx* ctx, const uint8_t* prev, size_t n, int prev_on_device);

/* ---- block-streaming entry points (host buffers; stream-major for n_streams > 1) ------ */
/* iq: n_streams x (n_blocks * block_bytes) u8; pcm: n_streams x (n_blocks * pcm_samples).  */
int fmrx_process(fmrx_ctx* ctx, const uint8_t* iq, size_t n_blocks, int16_t* pcm);
/* Split stages, the reference's thread split (project.cpp:19-85 | 87-197).
 * demod: n_streams x (n_blocks * if_samples) float.                                        */
int fmrx_rf_block(fmrx_ctx* ctx, const uint8_t* iq, size_t n_blocks, float* demod);
int fmrx_audio_block(fmrx_ctx* ctx, const float* demod, size_t n_blocks, int16_t* pcm);

/* ---- device-resident fused path (async on the context stream) ------------------------ */
/* Alignment, untuned u8 contexts: d_iq (and so every stream's row in it) may start at any byte and
 * d_pcm at any multiple of 2; rows that are not 16-byte aligned only cost one small launch more.
 * Tuned calls and the other formats are stricter (fmrx_set_input_format below).               */
int fmrx_process_device(fmrx_ctx* ctx, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm);
/* Optional float taps of the mono product (n_streams x n_blocks*audio_frames), may be NULL */
int fmrx_process_device_ex(fmrx_ctx* ctx, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm,
                           float* d_mono);
int fmrx_synchronize(fmrx_ctx* ctx);
void* fmrx_stream(fmrx_ctx* ctx);                       /* the hipStream_t used               */
/* Device time of the fused RF/demod/audio kernel, from HIP event pairs recorded around each
 * launch on the context stream (no host sync in between).  Returns the average over the
 * launches recorded since the last reset.  reset > 0: clear and arm recording; reset < 0:
 * clear and disarm; 0: just read.                                                         */
int fmrx_kernel_timing(fmrx_ctx* ctx, int reset, double* avg_ms, long* launches);

/* ---- off-centre tuning: several stations from one capture -------------------------------- */
/* A stream tuned to offset f Hz (integer, |f| < rf_fs/2) rotates its normalised I/Q pair n (the
 * absolute pair index of the stream) by e^(-j 2 pi f n / rf_fs) in front of the RF low-pass, so a
 * station at +f of the capture lands on 0 Hz; the rest of the chain is unchanged.  Arithmetic
 * (csrc/tuner.hip): N = rf_fs / gcd(|f|, rf_fs), k = (f / gcd) mod N, p = (k n) mod N,
 * I' = fl(fl(x_i c[p]) + fl(x_q s[p])), Q' = fl(fl(x_q c[p]) - fl(x_i s[p])) with the table below.
 * fmrx_tuner_design is host only, like fmrx_impulse_response_lpf: N, k and (cos_sin may be NULL)
 * the 2N floats c[0],s[0],c[1],s[1],..., c[p] = (float)cos(2 pi p / N), s[p] = (float)sin(2 pi p
 * / N) in double.  FMRX_EINVAL for |f| >= rf_fs/2 and for N > 4096 (any multiple of 1 kHz is
 * accepted in all four modes; cos_sin holds at most 8192 floats).                             */
int fmrx_tuner_design(int rf_fs, int offset_hz, int* N, int* k, float* cos_sin);
/* offsets_hz: n_streams ints, or NULL = tuning off (the untuned kernels run, exactly as today).
 * first_pair: absolute pair index of the next call's first I/Q pair (all streams).  Does not touch
 * filter/PLL/audio state.  A non-NULL array of zeros still takes the tuned front end.  While
 * tuning is on, fmrx_process, fmrx_process_device(_ex), fmrx_rf_block and the shared forms below
 * run the tuned front end, then the audio stage fmrx_audio_block runs (stereo contexts: the
 * non-pipelined engine), and advance the position by n_blocks * iq_pairs.  fmrx_reset keeps the
 * offsets and rewinds the position to 0.  Tuning is configuration, not state: the fmrx_get_state
 * blob does not hold it; a checkpoint is restored by fmrx_set_state plus fmrx_tune(..., first_pair)
 * with the position fmrx_tuner_info gave, and a time shard by fmrx_seek plus the same.
 * FMRX_EINVAL (nothing changed): an offset fmrx_tuner_design refuses.                          */
int fmrx_tune(fmrx_ctx* ctx, const int32_t* offsets_hz, uint64_t first_pair);
/* read back: offsets (n_streams, may be NULL), next pair index, 1/0 tuned (each may be NULL)  */
int fmrx_tuner_info(fmrx_ctx* ctx, int32_t* offsets_hz, uint64_t* next_pair, int* enabled);
/* one capture for every stream: iq is ONE stream's n_blocks*block_bytes, read by all n_streams
 * (each with its own offset); pcm as fmrx_process.  Tuning must be on (FMRX_ESTATE otherwise). */
int fmrx_process_shared(fmrx_ctx* ctx, const uint8_t* iq, size_t n_blocks, int16_t* pcm);
int fmrx_process_shared_device(fmrx_ctx* ctx, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm);

/* ---- raw I/Q formats: int8, int16 and float32 captures ------------------------------------------- */
/* The calls that take raw I/Q (fmrx_process, fmrx_process_device(_ex), fmrx_rf_block,
 * fmrx_process_shared(_device), fmrx_seek, fmrx_scan_spectrum(_device), fmrx_scan) read interleaved
 * pairs, I then Q, in the context's input format; their `const uint8_t*` is then the raw bytes of it.
 * The normalised samples x_i, x_q below are exact in float32 and take the place of the reference's
 * (u - 128) / 128 (src/iofunc.cpp:67) in front of everything else: with the tuner's table c, s
 * (fmrx_tune above) exactly I' = fl(fl(x_i c[p]) + fl(x_q s[p])), Q' = fl(fl(x_q c[p]) - fl(x_i s[p])),
 * then the RF FIR, the decimation and the discriminator as for u8 (csrc/tuner.hip rotates the
 * integers and applies the power of two once per RF output: DESIGN.md §5.7 says why that is exact).
 * For FMRX_IQ_F32 the bits are promised for samples that are 0 or of magnitude in [2^-20, 4];
 * anything else, NaN and Inf included, follows IEEE arithmetic and never faults.                   */
#define FMRX_IQ_U8  0   /* x = (u - 128) / 128       2 B a pair  (the default)                     */
#define FMRX_IQ_S8  1   /* x = s / 128               2 B a pair  int8                              */
#define FMRX_IQ_S16 2   /* x = s / 32768             4 B a pair  int16, little-endian              */
#define FMRX_IQ_F32 3   /* x = the float itself      8 B a pair  IEEE float32 (cf32)               */
/* bytes an I/Q pair of the format; host only; FMRX_EINVAL if unknown */
int fmrx_iq_pair_bytes(int format);
/* Sets the format of every stream of the context, then does what fmrx_reset does: the halo is
 * reallocated at its pair count times the pair's bytes and filled with the format's zero (0x80 for
 * u8, 0 otherwise), the offsets of fmrx_tune are kept, the position is rewound to 0.  Setting the
 * format the context already has is a reset and nothing else.  A block stays geo.iq_pairs pairs:
 * iq_pairs * fmrx_iq_pair_bytes(format) bytes (geo.block_bytes is the u8 figure), and every count
 * in bytes follows: fmrx_history_bytes, fmrx_seek's n (a whole number of pairs, FMRX_EINVAL
 * otherwise), the halo inside fmrx_state_size's blob (whose header records the format: a blob taken
 * in another format is refused with FMRX_ESTATE).  n_pairs of the scan stays a pair count.
 * With a format other than u8 every call that takes raw I/Q runs the tuned front end, also while
 * tuning is off: fmrx_tune(ctx, NULL, p) then means offset 0 for every stream (N = 1, c = 1, s = 0:
 * the bits of the untuned kernels); fmrx_process_shared* still needs an explicit fmrx_tune.  With
 * u8 nothing changes: tuning off runs the fused, untuned kernels.
 * Alignment: device pointers and row strides of those calls are aligned to two pairs (4, 4, 8, 16
 * bytes), the scan's d_iq to one pair (2, 2, 4, 8); anything less is FMRX_EINVAL and no launch.
 * FMRX_EINVAL, nothing changed: an unknown format; a format other than u8 where the mode and tap
 * count have no tuned kernel (rf_taps other than 51 and 101).
 * fmrx_normalize_iq, fmrx_synth_* and the RDS entry points stay u8 / float as they are.          */
int fmrx_set_input_format(fmrx_ctx* ctx, int format);
int fmrx_input_format(const fmrx_ctx* ctx, int* format);

/* ---- band scan: which offsets of a capture hold a station -------------------------------------- */
/* The step in front of fmrx_tune.  Spectrum (csrc/scan.hip): with x[n] = ((I_n - 128)
 * + j (Q_n - 128)) / 128 (u8; the context's input format's x_i + j x_q otherwise), N = fft_bins, nseg = n_pairs / N whole segments (no overlap, trailing pairs
 * ignored), w[i] = 0.5 - 0.5 cos(2 pi i / N) and X_s the N-point DFT of w . x_s,
 *     power[j] = 8 / (3 N^2 nseg) sum_s |X_s[(j - N/2) mod N]|^2,   j = 0 .. N-1:
 * linear power, FFT-shifted (bin j at (j - N/2) rf_fs / N Hz), sum_j power[j] ~ mean |x|^2, so 0 dB is
 * full scale on both rails.  A float32 estimate (within 0.01 dB a bin of the float64 value on 8-bit
 * captures), the same bits on every run.  The scan has scratch of its own in the context and does
 * not touch the receiver state: a scan between two fmrx_process calls leaves their output as it was.
 *
 * fmrx_scan_detect (host only, no context) on such a spectrum, everything in double:
 *   1. p[j] = max(power[j], 1e-20); kept bins: |j - N/2| >= dc_notch_bins;
 *   2. floor = element (floor_percentile (M - 1)) / 100 (integer division) of the M kept bins sorted
 *      ascending; *floor_db = 10 log10 floor;
 *   3. candidates f_m = raster_origin_hz + m raster_hz, every integer m with 2 |f_m| + channel_hz <= rf_fs;
 *   4. C_m = sum of p over the nb_m kept bins with 2 |(j - N/2) rf_fs - f_m N| <= channel_hz N (64-bit
 *      integers, no rounding); a candidate with nb_m = 0 is never reported;
 *   5. power_db = 10 log10 C_m, snr_db = 10 log10(C_m / (floor nb_m));
 *   6. candidates visited by C_m descending (ties: lower offset first); one is accepted when snr_db >=
 *      min_snr_db and it is at least min_separation_hz from every accepted one;
 *   7. *n_found = the number accepted; out gets the strongest max_out of them, ascending by offset_hz.
 * FMRX_EINVAL, nothing written: fft_bins no power of two in [256, 8192]; n_pairs < fft_bins; a
 * non-positive rf_fs, raster, channel or separation; channel_hz >= rf_fs; floor_percentile outside
 * 1..99; dc_notch_bins outside [0, fft_bins/2]; a candidate offset fmrx_tuner_design refuses (so every
 * reported offset can go straight into fmrx_tune).  cfg = NULL: the defaults.  fmrx_scan_detect takes the
 * transform size from its fft_bins argument, fmrx_scan from cfg->fft_bins.                          */
typedef struct {
    int fft_bins;            /* power of two in [256, 8192]; default 4096                     */
    int raster_hz;           /* channel raster; default 100000                                */
    int raster_origin_hz;    /* offset of one raster point from the capture centre; default 0 */
    int channel_hz;          /* integration bandwidth per candidate; default 150000           */
    int min_separation_hz;   /* between reported stations; default 200000                     */
    int dc_notch_bins;       /* bins j with |j - N/2| < this are ignored; default 1           */
    int floor_percentile;    /* 1..99, default 25                                             */
    float min_snr_db;        /* default 10                                                    */
} fmrx_scan_config;
typedef struct { int32_t offset_hz; float power_db; float snr_db; } fmrx_station;

int fmrx_scan_config_default(fmrx_scan_config* cfg);
/* host buffers; returns when power (fft_bins floats) is in host memory; n_segments may be NULL */
int fmrx_scan_spectrum(fmrx_ctx* ctx, const uint8_t* iq, size_t n_pairs, int fft_bins, float* power,
                       size_t* n_segments);
/* device buffers, async on the context stream; d_iq needs no alignment beyond one pair's bytes */
int fmrx_scan_spectrum_device(fmrx_ctx* ctx, const uint8_t* d_iq, size_t n_pairs, int fft_bins, float* d_power);
/* host only, no context (like fmrx_tuner_design); floor_db may be NULL */
int fmrx_scan_detect(const float* power, int fft_bins, int rf_fs, const fmrx_scan_config* cfg,
                     fmrx_station* out, int max_out, int* n_found, float* floor_db);
/* spectrum + detect with the context's rf_fs */
int fmrx_scan(fmrx_ctx* ctx, const uint8_t* iq, size_t n_pairs, const fmrx_scan_config* cfg,
              fmrx_station* out, int max_out, int* n_found);

/* ---- wide captures: a decimating down-converter ahead of the tuner ------------------------------- */
/* A capture at cap_fs = decim * rf_fs (decim an integer in 2..10; the radios deliver 8-20 MS/s) goes
 * through a per-station down-converter on the GPU (csrc/wide.hip) down to rf_fs, then
 * through the tuned front end of fmrx_tune unchanged.  An offset f Hz (|f| < cap_fs / 2) splits into
 *   q = sign(f) ((8 |f| + rf_fs) / (2 rf_fs)) (integer division), f_c = q rf_fs / 4, f_r = f - f_c,
 * so |f_r| <= rf_fs / 8.  Wide pair n (absolute index; x_i, x_q the format's normalised samples) is
 * rotated at the capture rate with N = 4 decim / gcd(|q|, 4 decim), k = (q / gcd) mod N, p = (k n) mod N
 * and the table of fmrx_tuner_design's form: I' = fl(fl(x_i c[p]) + fl(x_q s[p])), Q' = fl(fl(x_q c[p]) -
 * fl(x_i s[p])); then h = fmrx_impulse_response_lpf(cap_fs, 3 rf_fs / 8, 16 decim + 1, 1) and
 *   y[m] = sum_k h[k] (I', Q')[decim m - k], acc = fl(acc + fl(h[k] x)) from 0 in ascending k,
 * pairs in front of the stream being 0.  The pairs y[m] are a cf32 stream at rf_fs that takes the path
 * of an FMRX_IQ_F32 stream tuned to f_r, pair m at absolute index first_pair / decim + m.
 * fmrx_wide_design is host only: the split, N, k, the table (2 N <= 80 floats c0, s0, c1, s1, ...) and the
 * taps (*taps = 16 decim + 1 floats in h); every output pointer may be NULL.  FMRX_EINVAL, nothing
 * written: decim outside 2..10, rf_fs not a positive multiple of 4, |f| >= cap_fs / 2, a fine part
 * fmrx_tuner_design refuses (every multiple of 1 kHz passes).                                        */
int fmrx_wide_design(int rf_fs, int decim, int offset_hz, int* coarse_hz, int* fine_hz, int* N, int* k,
                     float* cos_sin, int* taps, float* h);
/* decim = 1 (the default): no wide stage.  2..10: allocates the wide state (the last 16 decim raw pairs
 * of the capture, the cf32 rows, an f32 halo for the narrow stage: all separate from what the ordinary
 * calls use), then does what fmrx_reset does.  The input format stays the capture's; a later
 * fmrx_set_input_format keeps decim.  FMRX_EINVAL: decim outside 1..10; no tuned kernel for the mode and
 * tap count (rf_taps other than 51 and 101).  While decim > 1, fmrx_get_state, fmrx_set_state and
 * fmrx_seek return FMRX_ESTATE; fmrx_reset clears the wide state too and keeps offsets and decim.
 * Changing decim turns wide tuning off (fmrx_tune_wide again); back at 1 the tuner keeps the fine
 * offsets fmrx_tune_wide gave it until the next fmrx_tune.                                           */
int fmrx_set_capture_decim(fmrx_ctx* ctx, int decim);
int fmrx_capture_decim(const fmrx_ctx* ctx, int* decim);
/* n_streams offsets against cap_fs; first_pair: absolute wide-pair index of the next call's first pair,
 * a multiple of decim (FMRX_EINVAL otherwise).  Stores the coarse tables and hands the fine parts and
 * first_pair / decim to the tuner state of fmrx_tune (fmrx_tuner_info then shows them; a later fmrx_tune
 * turns wide tuning off).  On any refusal nothing changes.  FMRX_ESTATE while decim is 1.             */
int fmrx_tune_wide(fmrx_ctx* ctx, const int32_t* offsets_hz, uint64_t first_pair);
/* read back: the wide offsets, the next absolute wide-pair index, 1/0 wide tuning (each may be NULL) */
int fmrx_wide_info(fmrx_ctx* ctx, int32_t* offsets_hz, uint64_t* next_pair, int* enabled);
/* ONE capture read by every stream: iq holds n_blocks blocks of decim * geo.iq_pairs wide pairs in the
 * context's input format; pcm as fmrx_process.  Any split of a capture into calls gives the same bits.
 * Long calls run in internal pieces of whole blocks, so the cf32 rows stay bounded.  Stereo contexts
 * take the non-pipelined engine.  FMRX_ESTATE without fmrx_tune_wide.  The device form is asynchronous
 * on the context stream; d_iq is aligned to two pairs of the format (FMRX_EINVAL and no launch
 * otherwise).  fmrx_kernel_timing, when armed, times the down-converter's launches.                 */
int fmrx_process_wide(fmrx_ctx* ctx, const uint8_t* iq, size_t n_blocks, int16_t* pcm);
int fmrx_process_wide_device(fmrx_ctx* ctx, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm);
/* fmrx_scan_detect with rf_fs := decim * rf_fs (bin j at (j - N/2) cap_fs / N Hz) and "a candidate
 * fmrx_wide_design refuses" in place of "fmrx_tuner_design refuses"; host only.                      */
int fmrx_scan_detect_wide(const float* power, int fft_bins, int rf_fs, int decim, const fmrx_scan_config* cfg,
                          fmrx_station* out, int max_out, int* n_found, float* floor_db);
/* fmrx_scan on a wide capture: the same spectrum kernel, then fmrx_scan_detect_wide with the context's
 * rf_fs and decim; every reported offset can go straight into fmrx_tune_wide.  FMRX_ESTATE at decim 1. */
int fmrx_scan_wide(fmrx_ctx* ctx, const uint8_t* iq, size_t n_pairs, const fmrx_scan_config* cfg,
                   fmrx_station* out, int max_out, int* n_found);

/* ---- captures at a rational rate: a polyphase down-converter ahead of the tuner ------------------- */
/* A capture at cap_fs Hz with rf_fs / cap_fs = L / M in lowest terms, 2 <= L <= 48, L < M <= 125,
 * M <= 10 L (10, 8, 20, 6, 3, 2.5, 12.5, 2.56, 3.2 MS/s against 2.4 MS/s; 2.048 against 1.152; ...) goes
 * through a rational down-converter on the GPU (csrc/rate.hip) down to rf_fs, then through
 * the tuned front end unchanged.  An offset f Hz (2 |f| < cap_fs) splits as in the wide section (q, f_c =
 * q rf_fs / 4, f_r = f - f_c).  Wide pair n is rotated at the capture rate with g = gcd(|q| L, 4 M),
 * N = 4 M / g <= 500, k = (q L / g) mod N (q = 0: N = 1, k = 0), p = (k n) mod N and the wide section's
 * formulas for I', Q'; then h = fmrx_impulse_response_lpf((float)rf_fs (float)M, 3 rf_fs / 8, 16 M + 1, L) and
 *   y[m] = sum h[k] (I', Q')[(m M - k) / L] over the k in 0..16 M with k = m M (mod L), ascending,
 *   acc = fl(acc + fl(h[k] x)) from 0, pairs in front of the stream being 0
 * (fmrx_resample's definition with up = L, down = M).  The pairs y[m] are a cf32 stream at rf_fs that takes
 * the path of an FMRX_IQ_F32 stream tuned to f_r, pair m at absolute index first_pair L / M + m.
 * fmrx_rate_design is host only: *up = L, *down = M, the split, N, k, the table (2 N <= 1000 floats) and
 * the taps (*taps = 16 M + 1 <= 2001 floats in h); every output pointer may be NULL.  An integer ratio
 * D = 2..10 answers as fmrx_wide_design does, with *up = 1, *down = D.  FMRX_EINVAL, nothing written:
 * rf_fs not a positive multiple of 4, cap_fs <= rf_fs, a ratio outside the limits, 2 |f| >= cap_fs, a fine
 * part fmrx_tuner_design refuses.                                                                     */
int fmrx_rate_design(int rf_fs, int cap_fs, int offset_hz, int* up, int* down, int* coarse_hz, int* fine_hz,
                     int* N, int* k, float* cos_sin, int* taps, float* h);
/* The capture's rate in Hz.  An integer ratio (L = 1; cap_fs = rf_fs is D = 1) does exactly what
 * fmrx_set_capture_decim(ctx, D) does.  A rational one allocates the rational wide state (the last
 * ceil(16 M / L) raw wide pairs, the taps, a 500-entry table a stream, and the cf32 rows and f32 halo of
 * the wide stage), then does what fmrx_reset does.  While it is set: fmrx_capture_decim reports 0;
 * fmrx_get_state, fmrx_set_state and fmrx_seek return FMRX_ESTATE; fmrx_set_input_format keeps the rate;
 * fmrx_set_capture_decim leaves it; fmrx_tune_wide, fmrx_wide_info, fmrx_process_wide(_device) and
 * fmrx_scan_wide serve it with their meanings, offsets against cap_fs and positions in wide pairs:
 * first_pair of fmrx_tune_wide is a multiple of M, and n_blocks of a wide call (still narrow blocks of
 * PCM out) a multiple of the granule's blocks (FMRX_EINVAL and no launch otherwise).  FMRX_EINVAL,
 * nothing changed: a rate fmrx_rate_design refuses, no tuned kernel for the mode and tap count, a
 * granule that is no whole number of two-pair staging units.                                          */
int fmrx_set_capture_rate(fmrx_ctx* ctx, int cap_fs);
/* read back (each may be NULL): the rate, L, M; an integer ratio D reads D rf_fs, 1, D */
int fmrx_capture_rate(const fmrx_ctx* ctx, int* cap_fs, int* up, int* down);
/* The unit of a wide call: B = L / gcd(L, geo.iq_pairs) narrow blocks = B geo.iq_pairs M / L wide pairs
 * (mode 0 at 10 MS/s: 3 and 80000); an integer ratio D reads 1 and D geo.iq_pairs.                    */
int fmrx_wide_granule(const fmrx_ctx* ctx, size_t* blocks, size_t* wide_pairs);
/* fmrx_scan_detect with rf_fs := cap_fs and "a candidate fmrx_rate_design(rf_fs, cap_fs, ...) refuses"
 * in place of "fmrx_tuner_design refuses"; host only.                                                 */
int fmrx_scan_detect_rate(const float* power, int fft_bins, int rf_fs, int cap_fs, const fmrx_scan_config* cfg,
                          fmrx_station* out, int max_out, int* n_found, float* floor_db);

/* ---- FM de-emphasis: the broadcast's 50 / 75 us pre-emphasis undone in front of the S16 quantiser -- */
/* Neither the reference nor, by default, this library de-emphasises.  The stage is defined here (csrc/
 * deemph.hip) so that it is exact in parallel.  audio_fs = if_fs audio_up / audio_down
 * (48000 in modes 0 and 1, 44100 in modes 2 and 3), tau_us 50 (most of the world) or 75 (the Americas,
 * Korea).  Taps, T = 64, in double: p = exp(-1.0 / (audio_fs tau_us 1e-6)), r[0] = 1 - p, r[n] = r[n-1] p,
 * h[n] = (float) r[n]: the one-pole filter's response, whose tail past 64 samples is below half a float32
 * ulp of its sum (p^64 <= 1.9e-8 < 2^-25 for these rates and time constants; a longer one would not be).
 * Filter, per stream and channel: y[n] = sum_k h[k] x[n - k], acc = fl(acc + fl(h[k] x)) from 0 in
 * ascending k (fmrx_resample's definition with up = down = 1), the 63 samples in front of a stream being
 * 0; then the quantiser of fmrx_quantize.  MONO contexts: x is the mono product.  STEREO contexts: left
 * and right (fmrx_lr_extraction's outputs) each go through the filter with a history of their own; the
 * PCM stays interleaved R, L.
 * fmrx_deemph_design is host only and needs no context, like fmrx_tuner_design: 64 floats into h64.
 * FMRX_EINVAL, nothing written: tau_us other than 50 and 75, audio_fs <= 0, h64 NULL.                 */
int fmrx_deemph_design(int audio_fs, int tau_us, float* h64);
/* tau_us 0 (the default): off -- no call does, launches or allocates anything more, every output bit is
 * what it was.  50 or 75: every call that writes PCM (fmrx_process, fmrx_process_device(_ex),
 * fmrx_audio_block, tuned calls, fmrx_process_shared(_device), fmrx_process_wide(_device); every mode,
 * mono and stereo, both stereo engines; with fmrx_set_rds too) routes the floats in front of its quantiser
 * into a scratch of the context -- 4 B per audio sample and channel of a call, grown on demand; a mono
 * fmrx_process_device_ex with d_mono uses that instead -- and the de-emphasis kernel then writes the
 * call's PCM.  d_mono of fmrx_process_device_ex stays the mono product as it was.  The carry (63 floats
 * per stream and channel) survives across calls, any split of a stream into calls gives the same bits;
 * fmrx_reset clears it and keeps the setting; fmrx_set_deemphasis (any value, the current one too) clears
 * it and nothing else.  While it is on, fmrx_get_state, fmrx_set_state and fmrx_seek return FMRX_ESTATE
 * (the blob does not hold the carry).  FMRX_EINVAL, nothing changed: any other tau_us.                */
int fmrx_set_deemphasis(fmrx_ctx* ctx, int tau_us);
int fmrx_deemphasis(const fmrx_ctx* ctx, int* tau_us);

/* ---- subcarrier meter: is there a 19 kHz pilot, is there a 57 kHz RDS subcarrier ------------------- */
/* No counterpart in the reference, which runs the pilot PLL on every stream (src/project.cpp:166).  The
 * meter says, per stream, whether the expensive stages have anything to lock to (csrc/meter.hip, DESIGN.md
 * §5.12).  It is stateless and defined exactly, so the GPU is checked without a tolerance.  Per stream on
 * the demod row d[n] at bp_fs: P = bp_fs / 1000 samples are a 1 ms window (240, 288, 240, 256 in modes
 * 0..3), 64 windows a frame (64 ms, the RDS window); a frame depends on its own 64 P samples alone.  Seven
 * tones at k kHz, k = 17, 19, 21, 56, 58, 61, 63 in that order: the pilot with the guard band either side
 * of it, the two sides of the RDS carrier (biphase RDS has a null at 57 kHz itself) and two bins above its
 * skirt.  fmrx_meter_design is host only, like fmrx_deemph_design; in double, then rounded to float:
 *   w[n] = 0.5 - 0.5 cos(2 pi n / P)                       (Hann: the pilot is an exact zero of 17 and 21)
 *   c_k[n] = (float)(w[n] cos(2 pi ((k n) mod P) / P)),  s_k[n] = (float)(w[n] sin(2 pi ((k n) mod P) / P))
 * tables: 7 x 2 x P floats, tone-major, c then s (may be NULL); *P may be NULL.  FMRX_EINVAL, nothing
 * written: bp_fs no positive multiple of 16000, or P > 288.
 * Per window and tone, x = d[window start + n]: sixteen partial sums a_j = fl(a_j + fl(x[16 i + j] c_k[16 i
 * + j])) from 0, i ascending over 0 .. P/16 - 1 (products and sums rounded separately, no FMA:
 * fmrx_resample's convention), folded by stride halving, a_j = fl(a_j + a_{j+s}) for j < s, s = 8, 4, 2, 1;
 * re = a_0, im the same with s_k, p = fl(fl(re re) + fl(im im)).  Per frame and tone the 64 window powers are
 * folded by the same tree (s = 32 .. 1).  power: n_streams x F x 7 floats, F the frames of the call.  NaN
 * and Inf in the input follow IEEE arithmetic and never fault.
 * A call takes whole frames: n_blocks a multiple of fmrx_rds_granule's blocks (24, 24, 3, 1; with a capture
 * rate set the least common multiple with fmrx_wide_granule's), else FMRX_EINVAL and nothing runs.         */
#define FMRX_METER_TONES 7
int fmrx_meter_design(int bp_fs, int* P, float* tables /* 14 P floats, may be NULL */);
/* the primitive: demod rows as fmrx_rf_block returns them, whole frames; power: n_streams x F x 7 */
int fmrx_meter(fmrx_ctx* ctx, const float* demod, size_t n_blocks, float* power);
int fmrx_meter_device(fmrx_ctx* ctx, const float* d_demod, size_t n_blocks,
                      float* d_power);             /* async on the context stream */
/* The decision, host only, no context, everything in double.  sum[t]: the sequential ascending sum, over
 * the frames in stream order, of the float powers widened to double (any split of a stream into calls
 * gives the same bits).  With S19 = max(sum[19], 1e-30), R = (sum[56] + sum[58]) / 2:
 *   pilot_snr_db = 10 log10(S19 / max((sum[17] + sum[21]) / 2, 1e-30)),  pilot_db = 10 log10(S19 / (64 frames))
 *   rds_snr_db = 10 log10(max(R, 1e-30) / max((sum[61] + sum[63]) / 2, 1e-30)),  rds_db = 10 log10(max(R, 1e-30) / (64 frames))
 *   stereo = pilot_snr_db >= cfg.pilot_min_snr_db,  rds = rds_snr_db >= cfg.rds_min_snr_db
 * (defaults 10 dB and 1.94 dB, DESIGN.md §5.12 has the measured classes either side; cfg = NULL: the
 * defaults).  FMRX_EINVAL: a null report or out, frames == 0.                                              */
typedef struct { double sum[FMRX_METER_TONES]; uint64_t frames; } fmrx_meter_report;
typedef struct { float pilot_min_snr_db, rds_min_snr_db; } fmrx_meter_config;
typedef struct { float pilot_db, pilot_snr_db, rds_db, rds_snr_db;
                 int stereo, rds; } fmrx_subcarriers;
int fmrx_meter_config_default(fmrx_meter_config* cfg);
int fmrx_meter_accumulate(fmrx_meter_report* io, const float* power,
                          size_t frames);          /* host only: frames x 7 floats of one stream */
int fmrx_meter_detect(const fmrx_meter_report* report, const fmrx_meter_config* cfg,
                      fmrx_subcarriers* out);
/* on != 0: the calls whose front end writes demod rows (tuned fmrx_process / _device / _device_ex,
 * fmrx_process_shared / _device, fmrx_process_wide / _device) also run the meter over those rows, on the
 * context stream in front of the audio stage, copy the F x 7 floats a stream back and add them to the
 * stream's report once the call's work is enqueued (a host synchronisation, as with fmrx_set_rds).  Such a
 * call must be whole frames (FMRX_EINVAL and nothing runs otherwise).  The PCM is the same bits either
 * way.  fmrx_reset clears the reports and keeps the switch; the reports are not in the fmrx_get_state blob
 * (the meter holds no signal state).  Off (the default): no call launches, allocates or copies anything
 * more.  The untuned fused u8 path writes no demod rows and is never metered.                             */
int fmrx_set_meter(fmrx_ctx* ctx, int on);
int fmrx_meter_get(const fmrx_ctx* ctx, int stream, fmrx_meter_report* out);

/* ---- soft stereo: every stereo stream blended toward mono by its pilot's signal-to-noise ratio ------ */
/* No counterpart in the reference.  The L-R channel carries about 20 dB more noise than L+R, so a receiver
 * blends a weak station toward mono instead of switching (csrc/blend.hip).  The stage is
 * defined exactly -- float32 throughout, products and sums rounded separately, no FMA -- so the GPU is
 * checked without a tolerance.  A call is a whole number of RDS granules (fmrx_rds_granule: 24, 24, 3, 1
 * blocks in modes 0..3); a granule holds Gm = 1, 1, 20, 20 meter frames and A = 3072, 3072, 56448, 56448
 * audio frames.
 * Thresholds (fmrx_blend_design: host only, no context, in double until stored):
 *   T[j] = (float)(0.5 * 10^((lo_db + j (hi_db - lo_db) / 15) / 10)),  j = 0..15
 * (the 0.5 folds the mean of the two guard bins into the threshold).  Both bounds finite, in [-20, 60],
 * lo_db < hi_db, else FMRX_EINVAL and nothing written; defaults 10 and 22 dB.
 * Levels, per stream and meter frame f counted from the last fmrx_reset, from the meter's power[f][tone]:
 *   a_f = power[f][19 kHz],  g_f = fl(power[f][17 kHz] + power[f][21 kHz]),  both 0 for f < 0
 *   S_f = fl(fl(fl(a_{f-3} + a_{f-2}) + a_{f-1}) + a_f),  G_f the same over g
 *   l_f = #{ j : S_f >= fl(T[j] G_f) }  in 0..16 (a NaN compares false),  l_{-1} = 0
 * so a stream starts mono and ramps up.  Carry, 8 floats a stream: a_{f-3}, a_{f-2}, a_{f-1}, g_{f-3}, g_{f-2},
 * g_{f-1} of the next frame f, the last level as a float (anything outside 0..16 counts as 0), 0.  Zeros
 * are the power-on state; any split of a stream into calls gives the same levels.
 * Apply, for audio frame n of a stream counted from the reset, all in integers:
 *   r = n / A,  a = n mod A,  u = a Gm,  f = r Gm + u / A,  t = u mod A,  q = l_{f-1} (A - t) + l_f t
 *   k = fl((float)(16 A - q) c),  c = (float)(1.0 / (32.0 A))
 * With (R, L) the floats in front of the quantiser: where q == 16 A the pair passes bit for bit; elsewhere
 * d = fl(L - R), e = fl(k d), L' = fl(L - e), R' = fl(R + e): k = 0 is full stereo, k = 0.5 mono.  The result
 * goes to de-emphasis if that is on, otherwise to fmrx_quantize's quantiser; the PCM stays interleaved R, L.
 * (The sign and payload of a NaN that the arithmetic itself makes, Inf - Inf, are IEEE 754's to leave open and
 * stay open here; the quantiser sends every NaN to 0.)                                                  */
typedef struct { float lo_db, hi_db; } fmrx_blend_config;
typedef struct { uint64_t frames; uint64_t level_frames[17]; } fmrx_blend_report;   /* frames at each level */
int fmrx_blend_config_default(fmrx_blend_config* cfg);
int fmrx_blend_design(const fmrx_blend_config* cfg /* NULL: defaults */, float* T16);
/* The levels primitive, any F >= 1.  power: n_streams x F x 7 (fmrx_meter's); carry: n_streams x 8 floats,
 * in and out; levels: n_streams x (F + 1) bytes, entry 0 the carried-in level, entry 1 + f frame f's.      */
int fmrx_blend_levels(fmrx_ctx* ctx, const fmrx_blend_config* cfg, const float* power, size_t F, float* carry,
                      uint8_t* levels);
int fmrx_blend_levels_device(fmrx_ctx* ctx, const fmrx_blend_config* cfg, const float* d_power, size_t F,
                             float* d_carry, uint8_t* d_levels);   /* async on the context stream */
/* The apply primitive (STEREO contexts; async on the context stream).  d_rl: n_streams rows of n (R, L)
 * float pairs, n a whole number of granules' audio frames, the first being frame 0 of a granule, 16-byte
 * aligned; d_levels: n_streams rows of n Gm / A + 1 bytes as fmrx_blend_levels writes them (values 0..16);
 * d_out: the blended floats (may be NULL, may be d_rl); d_pcm: their S16 (may be NULL).                   */
int fmrx_blend_apply_device(fmrx_ctx* ctx, const float* d_rl, size_t n, const uint8_t* d_levels, float* d_out,
                            int16_t* d_pcm);
/* on != 0 (STEREO contexts; FMRX_EINVAL on a MONO one): the calls whose front end writes demod rows (tuned
 * fmrx_process / _device / _device_ex, fmrx_process_shared / _device, fmrx_process_wide / _device) run the
 * meter kernel over those rows (one launch, shared with fmrx_set_meter, whose reports are what they were),
 * the levels kernel behind it, route the (right, left) floats in front of the quantiser into the scratch
 * de-emphasis uses and run the apply kernel on them; the level bytes are copied back once the call's work
 * is enqueued (a host synchronisation, as with fmrx_set_meter) and counted in the stream's report.  Such a
 * call must be whole granules (FMRX_EINVAL and nothing runs otherwise).  While it is on, the calls without
 * demod rows -- untuned fmrx_process / _device / _device_ex and fmrx_audio_block -- return FMRX_ESTATE,
 * launch nothing and leave their output untouched (fmrx_tune(ctx, zeros, pos) gives the untuned bits
 * through the tuned front end), and so do fmrx_get_state, fmrx_set_state and fmrx_seek (the blob does not
 * hold the carry).  cfg NULL: the defaults; a bad cfg: FMRX_EINVAL, nothing changed.  fmrx_reset clears the
 * carry and the reports and keeps the switch and the config; fmrx_set_stereo_blend, with any value, clears
 * the carry and the reports and changes nothing else.  Off (the default): no call launches, allocates or
 * copies anything more, every output bit is what it was.                                                 */
int fmrx_set_stereo_blend(fmrx_ctx* ctx, int on, const fmrx_blend_config* cfg /* NULL: defaults */);
int fmrx_stereo_blend(const fmrx_ctx* ctx, int* on, fmrx_blend_config* cfg);
/* The end of a stream that is no whole granule (the CLI's last blocks).  on != 0, with soft stereo on (else
 * FMRX_ESTATE): the blended calls take any block count and run the apply kernel at every stream's last
 * level throughout (l_{f-1} = l_f = the level of the last frame counted, 0 after a reset); the meter and
 * the levels kernel do not run for the stage, the carry and the reports stay as they are.  fmrx_reset and
 * fmrx_set_stereo_blend turn it off.                                                                     */
int fmrx_blend_hold(fmrx_ctx* ctx, int on);
int fmrx_blend_get(const fmrx_ctx* ctx, int stream, fmrx_blend_report* out);

/* ---- quieting: high-cut and soft mute from every stream's noise level -------------------------------- */
/* No counterpart in the reference.  As a station weakens a broadcast receiver first rolls off the treble
 * (high-cut) and finally turns the audio down (soft mute); here both follow the discriminator noise in the
 * meter's 61 and 63 kHz bins, above the RDS skirt, where no programme content lives and the noise depends on
 * the carrier-to-noise ratio alone (csrc/quiet.hip).  MONO and STEREO contexts alike.  The
 * stage is defined exactly -- float32 throughout, products and sums rounded separately, no FMA -- so the
 * GPU is checked without a tolerance.  A call is a whole number of RDS granules, as for soft stereo
 * (fmrx_rds_granule: 24, 24, 3, 1 blocks in modes 0..3; with a capture rate set the least common multiple
 * with fmrx_wide_granule's); a granule holds Gm = 1, 1, 20, 20 meter frames and A = 3072, 3072, 56448, 56448
 * audio frames.  The defaults below rest on synthetic stations (DESIGN.md §5.16 has the table); nobody has
 * measured them on an off-air capture.
 * Config: cut_lo_db, cut_hi_db: the readings (dB) at which the high-cut begins and is complete; mute_lo_db,
 * mute_hi_db: the same for the soft mute; mute_depth_db: how far the mute turns the audio down; corner_hz:
 * the high-cut's corner.  Defaults 22, 34, 36, 44, 20, 2500.  Valid: every float finite, each lo < hi, all
 * four bounds in [-40, 80], 0 <= mute_depth_db <= 60, corner_hz <= 8000 and exp(-128 pi corner_hz / audio_fs)
 * < 2^-25 (the 64-tap bound of de-emphasis: corner_hz >= 2069 at 48 kHz, >= 1901 at 44.1 kHz); anything else:
 * FMRX_EINVAL, nothing changed.
 * Design (fmrx_quiet_design: host only, no context, in double until stored; audio_fs 48000 or 44100, which
 * fixes A = 3072 or 56448, bp_fs as fmrx_meter_design takes it), with P = bp_fs / 1000:
 *   Tc[j] = (float)(4 (P / 240.0) 10^((cut_hi_db - j (cut_hi_db - cut_lo_db) / 15) / 10)),  j = 0..15
 *   Tm[j] the same over the mute bounds;  h[64]: fmrx_deemph_design's recipe with p = exp(-2 pi corner_hz /
 *   audio_fs);  g0 = (float)10^(-mute_depth_db / 20),  cg = (float)((1.0 - (double)g0) / (16.0 A)),
 *   cw = (float)(1.0 / (16.0 A))
 * (a reading is 10 log10(N / 4 / (P / 240)) dB of the four-frame sum N below).  Every output pointer may be
 * NULL; g0_cg_cw takes the three gains in that order.
 * Levels, per stream and meter frame f counted from the last fmrx_reset, from the meter's power[f][tone]:
 *   n_f = fl(power[f][61 kHz] + power[f][63 kHz]),  0 for f < 0
 *   N_f = fl(fl(fl(n_{f-3} + n_{f-2}) + n_{f-1}) + n_f)
 *   c_f = #{ j : N_f <= Tc[j] },  m_f = #{ j : N_f <= Tm[j] }   both in 0..16, 16: untouched (a NaN compares
 *   false and closes the stream),  c_{-1} = m_{-1} = 0
 * so a stream starts closed and fades in over its first frame, as a squelch opens.  Carry, 8 floats a
 * stream: n_{f-3}, n_{f-2}, n_{f-1} of the next frame f, the last c and m as floats (anything outside 0..16
 * counts as 0), three zeros.  Zeros are the power-on state; any split of a stream into calls gives the same
 * levels.
 * Apply, for audio frame n of a stream counted from the reset, in integers:
 *   r = n / A,  a = n mod A,  u = a Gm,  f = r Gm + u / A,  t = u mod A
 *   qc = c_{f-1} (A - t) + c_f t,  qm = m_{f-1} (A - t) + m_f t
 * On a STEREO context R and L each take the two steps with a history of their own and the same levels.  For
 * a sample x of the floats in front of the quantiser:
 *   1. high-cut.  qc == 16 A: y = x bit for bit, a NaN's payload included.  Elsewhere v = sum_k h[k] x[n - k],
 *      acc = fl(acc + fl(h[k] x[n - k])) from 0 in ascending k (the 63 inputs in front of a stream are 0);
 *      w = fl((float)(16 A - qc) cw),  d = fl(v - x),  e = fl(w d),  y = fl(x + e)
 *   2. soft mute.  qm == 16 A: z = y bit for bit.  Elsewhere g = fl(g0 + fl((float)qm cg)),  z = fl(g y)
 * z goes to de-emphasis if that is on, otherwise to fmrx_quantize's quantiser; stereo PCM stays interleaved
 * R, L.  With soft stereo on too the order is blend, quieting, de-emphasis, quantiser.  The stage carries 63
 * floats of its input per stream and channel across calls.  (The sign and payload of a NaN that the
 * arithmetic itself makes stay open, as with soft stereo; the quantiser sends every NaN to 0.)  A stream
 * whose levels are all 16 gives the stage-off PCM from its second meter frame on.                          */
typedef struct { float cut_lo_db, cut_hi_db, mute_lo_db, mute_hi_db, mute_depth_db; int corner_hz; } fmrx_quiet_config;
typedef struct { uint64_t frames; uint64_t cut_frames[17]; uint64_t mute_frames[17]; } fmrx_quiet_report;
int fmrx_quiet_config_default(fmrx_quiet_config* cfg);
int fmrx_quiet_design(int audio_fs, int bp_fs, const fmrx_quiet_config* cfg /* NULL: defaults */, float* Tc16, float* Tm16,
                      float* h64, float* g0_cg_cw /* 3 */);
/* The levels primitive, any F >= 1.  power: n_streams x F x 7 (fmrx_meter's); carry: n_streams x 8 floats,
 * in and out; levels: n_streams x 2 (F + 1) bytes, pair e = (c, m): pair 0 the carried-in one, pair 1 + f
 * frame f's.                                                                                              */
int fmrx_quiet_levels(fmrx_ctx* ctx, const fmrx_quiet_config* cfg, const float* power, size_t F, float* carry,
                      uint8_t* levels);
int fmrx_quiet_levels_device(fmrx_ctx* ctx, const fmrx_quiet_config* cfg, const float* d_power, size_t F,
                             float* d_carry, uint8_t* d_levels);   /* async on the context stream */
/* The apply primitive (async on the context stream), with the taps and gains of the context's config
 * (fmrx_set_quieting's, the defaults before it).  d_in: n_streams rows of n frames (STEREO: (R, L) pairs), n
 * a whole number of granules' audio frames, the first being frame 0 of a granule; d_levels: n_streams rows
 * of 2 (n Gm / A + 1) bytes as fmrx_quiet_levels writes them (values 0..16); d_state: n_streams x channels x
 * 63 floats, the inputs in front of the call, in and out; d_out: the floats (may be NULL), d_pcm: their S16
 * (may be NULL), both laid out as d_in; one of the two at least.  Not in place (workgroups read their
 * neighbours' inputs): FMRX_EINVAL where d_out overlaps d_in.                                              */
int fmrx_quiet_apply_device(fmrx_ctx* ctx, const float* d_in, size_t n, const uint8_t* d_levels, float* d_state,
                            float* d_out, int16_t* d_pcm);
/* on != 0: the calls whose front end writes demod rows (tuned fmrx_process / _device / _device_ex,
 * fmrx_process_shared / _device, fmrx_process_wide / _device) run the meter kernel over those rows (one
 * launch, however many of fmrx_set_meter, soft stereo and quieting are on; the meter's reports are what they
 * were), the levels kernel behind it, and the apply kernel on the floats in front of the quantiser: it writes
 * the PCM itself when de-emphasis is off and a scratch of its own, which de-emphasis then reads, when it is
 * on.  d_mono of a mono fmrx_process_device_ex is read and never written: it stays the mono product as it
 * was.  The level bytes are copied back once the call's work is enqueued (a host synchronisation, as with
 * fmrx_set_meter) and counted in the stream's report.  Such a call must be whole granules (FMRX_EINVAL and
 * nothing runs otherwise).  While it is on, the calls without demod rows -- untuned fmrx_process / _device /
 * _device_ex and fmrx_audio_block -- return FMRX_ESTATE, launch nothing and leave their output untouched,
 * and so do fmrx_get_state, fmrx_set_state and fmrx_seek (the blob holds neither carry).  cfg NULL: the
 * defaults; a bad cfg: FMRX_EINVAL, nothing changed.  fmrx_reset clears both carries and the reports and
 * keeps the switch and the config; fmrx_set_quieting, with any value, clears both carries and the reports
 * and changes nothing else.  Off (the default): no call launches, allocates or copies anything more, every
 * output bit is what it was.                                                                             */
int fmrx_set_quieting(fmrx_ctx* ctx, int on, const fmrx_quiet_config* cfg /* NULL: defaults */);
int fmrx_quieting(const fmrx_ctx* ctx, int* on, fmrx_quiet_config* cfg);
/* The end of a stream that is no whole granule, fmrx_blend_hold's analogue.  on != 0, with quieting on (else
 * FMRX_ESTATE): the calls take any block count and run the apply kernel at every stream's last levels
 * throughout (those of the last frame counted, 0 after a reset); the meter and the levels kernel do not run
 * for the stage, the level carry and the reports stay as they are; the FIR history still moves.  fmrx_reset
 * and fmrx_set_quieting turn it off.                                                                      */
int fmrx_quiet_hold(fmrx_ctx* ctx, int on);
int fmrx_quiet_get(const fmrx_ctx* ctx, int stream, fmrx_quiet_report* out);

/* ---- AFC: measure each stream's carrier offset and retune to it -------------------------------------- */
/* No counterpart in the reference, which decodes a station at the capture's centre.  A scan reports offsets
 * on a raster and a real capture is never on it (crystal error, the capture's centre), so the demod row of a
 * tuned stream carries the tuning error as its mean (csrc/afc.hip).  The sums are stateless
 * and defined exactly, so the GPU is checked without a tolerance.  Per stream and frame of the demod row
 * d[n] (the meter's frame: 64 windows of P = bp_fs / 1000 samples, 64 ms), two floats: S, the sum of d[n],
 * and Q, the sum of fl(d[n] d[n]).  Per window, x = d[window start + n]: sixteen partial sums each,
 *   a_j = fl(a_j + x[16 i + j]),  b_j = fl(b_j + fl(x[16 i + j] x[16 i + j]))   from 0, i ascending over 0 .. P/16 - 1
 * (products and sums rounded separately, no FMA), folded by stride halving, a_j = fl(a_j + a_{j+s}) for
 * j < s, s = 8, 4, 2, 1; the frame's 64 window values a_0 (b_0) are folded by the same tree (s = 32 .. 1).
 * sums: n_streams x F x 2 floats (S, Q), F the frames of the call.  NaN and Inf in the input follow IEEE
 * arithmetic, stay in their frame and never fault.  A call takes whole frames, fmrx_meter's granule rule:
 * else FMRX_EINVAL, nothing launched, nothing written.  The device form's rows are 16-byte aligned
 * (FMRX_EINVAL otherwise).                                                                                */
int fmrx_carrier(fmrx_ctx* ctx, const float* demod, size_t n_blocks, float* sums);
int fmrx_carrier_device(fmrx_ctx* ctx, const float* d_demod, size_t n_blocks,
                        float* d_sums);            /* async on the context stream */
/* sum, sumsq: the sequential ascending sums, over the frames in stream order, of S and of Q widened to
 * double (any split of a stream into calls gives the same bits).                                           */
typedef struct { double sum, sumsq; uint64_t frames; } fmrx_carrier_report;
int fmrx_carrier_accumulate(fmrx_carrier_report* io, const float* sums,
                            size_t frames);        /* host only: frames x 2 floats of one stream */
/* The decision, host only, no context, everything in double.  With n = 64 P frames samples (P = bp_fs /
 * 1000), mean = sum / n and mean_square = sumsq / n:
 *   err_hz = asin(clamp(mean, -1, 1)) bp_fs / (2 pi)         (positive: the carrier is above the tuned offset)
 *   carrier = mean_square <= cfg.max_mean_square
 *   correction_hz = step_hz round_half_away(err_hz / step_hz) if carrier and |err_hz| >= deadband_hz, else 0
 * The discriminator returns the sine of the phase step, so err_hz is exact for an unmodulated carrier;
 * modulation shrinks the reading by E[cos m] (J0(beta) for a tone: 0.98 for a quiet multiplex, 0.22 at 75 kHz
 * tone deviation, positive below about 92 kHz), so repeated decisions close in on the carrier and do not
 * overshoot.  A constant-envelope signal has |d| <= 1, noise alone has heavy tails (mean squares of 3.5 to
 * 8.5 on synthetic captures): the gate's default of 1.0 is that bound, not a tuned value.
 * Defaults: step_hz 1000 (the grid on which fmrx_tuner_design accepts every offset in every mode),
 * deadband_hz 1000, max_pull_hz 50000 (half the scan's default raster), frames 16 (about a second), track 1,
 * max_mean_square 1.0.  They rest on synthetic stations; no off-air capture has been through them.
 * FMRX_EINVAL, nothing written: a null argument, step_hz, frames or max_pull_hz <= 0, deadband_hz < 0,
 * max_mean_square not finite or <= 0, bp_fs no positive multiple of 16000, a report of 0 frames.  cfg NULL:
 * the defaults.                                                                                            */
typedef struct { int step_hz, deadband_hz, max_pull_hz, frames, track; float max_mean_square; } fmrx_afc_config;
typedef struct { double err_hz, mean, mean_square; int carrier; int32_t correction_hz; } fmrx_afc_decision;
int fmrx_afc_config_default(fmrx_afc_config* cfg);
int fmrx_afc_decide(const fmrx_carrier_report* report, int bp_fs, const fmrx_afc_config* cfg,
                    fmrx_afc_decision* out);
/* on != 0: the calls whose front end writes demod rows (tuned fmrx_process / _device / _device_ex,
 * fmrx_process_shared / _device, fmrx_process_wide / _device) also run the carrier sums over those rows, on
 * the context stream behind the meter, the blend levels and RDS, copy the F x 2 floats a stream back and add
 * them to two reports a stream once the call's work is enqueued (a host synchronisation, as with
 * fmrx_set_meter): the stream's total and the window since its last decision.  Such a call must be whole
 * frames (FMRX_EINVAL and nothing runs otherwise).  The PCM of the call is the same bits either way.
 * With cfg.track != 0, when the call's work is finished every stream whose window holds at least cfg.frames
 * frames gets fmrx_afc_decide's decision over the whole window, and the window is cleared.  Its new offset
 * is the current one plus the correction, clamped to origin +- max_pull_hz, origin being the offset the
 * caller last gave fmrx_tune or fmrx_tune_wide for the stream (on a context with a capture stage, once
 * fmrx_tune_wide was accepted, the offsets are the ones against the capture's rate).  If any stream moved,
 * the context retunes all streams at its current position, as fmrx_tune (fmrx_tune_wide) with
 * fmrx_tuner_info's (fmrx_wide_info's) position would; the next call starts on the new tables.  A new
 * offset the design refuses leaves that stream where it was and is counted in `refused`.  Retunes happen
 * at call boundaries only, so WITH TRACKING THE PCM DEPENDS ON HOW A STREAM IS SPLIT INTO CALLS; with
 * track == 0 (measure only) nothing depends on the split.  A caller's own fmrx_tune / fmrx_tune_wide sets
 * new origins and clears the windows; fmrx_reset puts the offsets back to the origins, clears the reports,
 * the decisions and the counts and keeps the switch and the config; none of it is in the fmrx_get_state
 * blob, as with tuning.  fmrx_set_afc with on != 0 clears the reports, the decisions and the counts (on == 0
 * leaves them readable); either leaves the offsets and the origins where they are.  cfg NULL: the defaults; a bad
 * cfg: FMRX_EINVAL, nothing changed.  Off (the default): no call launches, allocates or copies anything more,
 * every output bit is what it was.  The untuned fused u8 path and fmrx_audio_block write no demod rows and
 * are never measured.                                                                                       */
typedef struct { fmrx_carrier_report total; int32_t origin_hz, offset_hz; uint32_t retunes, refused;
                 uint32_t decisions; fmrx_afc_decision last; /* zeros before the first decision */
               } fmrx_afc_status;
int fmrx_set_afc(fmrx_ctx* ctx, const fmrx_afc_config* cfg /* NULL: defaults */, int on);
int fmrx_afc_get(const fmrx_ctx* ctx, int stream, fmrx_afc_status* out);

/* ---- filter.h primitives on device buffers (context stream; s = per-call state) ------- */
/* What holds for all of them: any taps, up, down >= 1 and any n >= 0, device pointers aligned to their
 * element only (4 bytes for float, 1 for the I/Q bytes).  n = 0 is a no-op: FMRX_OK, nothing written,
 * the carried state as it was (fmrx_pll too).  A null pointer, a negative n, or taps, up or down < 1 is
 * FMRX_EINVAL with nothing launched.  In place: fmrx_mixer (d_out = d_a or d_b), fmrx_lr_extraction
 * (d_left, d_right = d_mono, d_stereo in either order) and fmrx_pll (always) run in place, since an element
 * depends on itself only.  fmrx_resample (d_out = d_in), fmrx_fm_demod and fmrx_fm_demod_arctan
 * (d_out = d_i or d_q), fmrx_quantize (d_out = d_x) and fmrx_deemph (d_out = d_in) do not, an output
 * lying where another thread still reads: FMRX_EINVAL.  Only equal pointers are refused; buffers that
 * overlap in part are the caller's responsibility.                                             */
int fmrx_impulse_response_lpf(float* h, float fs, float fc, int taps, int gain);      /* host */
int fmrx_impulse_response_bpf(float* h, float fs, float fb, float fe, int taps);      /* host */
/* d_state: taps-1 floats (in/out): the inputs in front of d_in[0], afterwards the last taps-1 of d_in,
 * whatever the output count.  n_in >= taps-1 (a shorter call would have to keep part of the old state:
 * FMRX_EINVAL).  Returns the output count n_in up / down, which may be 0, in *n_out.  Phases without a
 * tap (taps < up) give 0.0.                                                                   */
int fmrx_resample(fmrx_ctx* ctx, float* d_out, float* d_state, const float* d_in, int n_in,
                  const float* d_coeff, int taps, int up, int down, int* n_out);
/* The de-emphasis kernel on one row, with the context's audio rate's taps for tau_us (50 or 75, whatever
 * fmrx_set_deemphasis says): y = the filter above over d_in[0..n), d_state the 63 floats in front of them
 * (in/out: afterwards the last 63 of state ++ input, n may be shorter than that).  d_out gets y, d_pcm its
 * quantised form; each may be NULL; d_out must not be d_in.                                         */
int fmrx_deemph(fmrx_ctx* ctx, const float* d_in, size_t n, int tau_us, float* d_state /* 63 floats, in/out */,
                float* d_out /* may be NULL */, int16_t* d_pcm /* may be NULL */);
/* d_prev: 2 floats {prev_i, prev_q} (in/out; n = 0 leaves them).  d_out must be neither d_i nor d_q. */
int fmrx_fm_demod(fmrx_ctx* ctx, float* d_out, float* d_prev, const float* d_i,
                  const float* d_q, int n);
/* d_io: PLL input, overwritten by the NCO output.  d_st: 6 floats {integrator, phaseEst,
 * feedbackI, feedbackQ, ncoOut_state, trigOffset} (in/out).  Every PLL (this call, stereo,
 * RDS) runs speculatively with the same bits as the certified recurrence: below trigOffset
 * 2^17 (and without a known trigOffset) the serial loop runs uncertified and every 16-sample
 * batch is re-verified exactly in parallel, the certified path resuming from the first batch
 * that differs; from 2^17 the self-certifying runners (index, three-wave) prove each step as
 * they go and redo a missed interval exactly themselves.  Knob FMRX_KNOB_PLL_SPEC 0 selects the
 * plain certified launch.  fmrx_pll reads d_st's trigOffset back (4 bytes, a host
 * synchronisation on the context stream) to choose the runners.                             */
int fmrx_pll(fmrx_ctx* ctx, float* d_io, int n, float freq, float fs, float nco_scale,
             float phase_adjust, float norm_bw, float* d_st);
int fmrx_mixer(fmrx_ctx* ctx, float* d_out, const float* d_a, const float* d_b, int n);
int fmrx_lr_extraction(fmrx_ctx* ctx, float* d_left, float* d_right, const float* d_mono,
                       const float* d_stereo, int n);
/* u8 interleaved I,Q -> float I and Q (n_pairs each), iofunc.cpp:67 normalisation.        */
int fmrx_normalize_iq(fmrx_ctx* ctx, const uint8_t* d_iq, size_t n_pairs, float* d_i, float* d_q);
/* S16 quantiser of project.cpp:185-191 (NaN -> 0, x86 truncation + 16-bit wrap).  d_out must not be
 * d_x: output k lies in input k / 2.                                                          */
int fmrx_quantize(fmrx_ctx* ctx, const float* d_x, size_t n, int16_t* d_out);

/* ---- RDS front half (rds_thread body, src/project.cpp:200-271) ------------------------- */
/* demod (IF rate, as fmrx_rf_block returns it) -> BPF 54-60 kHz -> square -> BPF
 * 113.5-114.5 kHz -> PLL(114 kHz, bp_fs, ncoScale 0.5, 0, 0.01) -> 5-sample channel delay ->
 * mixer.  Every buffer is n_streams x (n_blocks * if_samples) float; rds is the mixer output
 * (project.cpp:271 mixer_data), nco the PLL output (:259), channel the 54-60 kHz band (:247);
 * nco and channel may be NULL.  The RDS state (filter histories, PLL, delay line) lives in the
 * context, starts as the reference's (:206-226), is cleared by fmrx_reset and is not part of
 * the fmrx_get_state blob.  Block-size invariant: any n_blocks per call.                     */
int fmrx_rds_block(fmrx_ctx* ctx, const float* demod, size_t n_blocks, float* rds, float* nco,
                   float* channel);
int fmrx_rds_device(fmrx_ctx* ctx, const float* d_demod, size_t n_blocks, float* d_rds,
                    float* d_nco, float* d_channel);

/* ---- RDS back half: bits, block sync and station name ------------------- */
/* The reference stops at the mixer output; what follows has no counterpart there.  Per stream:
 *   1. y = resample(rds, impulseResponseLPF(19 bp_fs, 3000, 101 x 19, 19), 19, bp_fs / 2000) from
 *      zero state: 38,000 S/s in every mode (16 samples a biphase chip), the reference's own resample
 *      and the only floating-point stage;
 *   2. signs s[n] = (y[n] >= 0), 1 in front of the stream;
 *   3. per window of 2432 samples (76 bits): sign changes counted by n mod 16, z the lowest index of
 *      the largest bin, phase p = (z + 8) mod 16, chips c[j] = s[2432 w + p + 16 j], j < 152;
 *   4. e = [the chip in front of the window (1 in front of the stream), c]: v0 equal pairs
 *      (e[2i], e[2i+1]), v1 equal pairs (e[2i+1], e[2i+2]), i < 76; q = (v1 > v0); the symbols are
 *      e[2i+1] for q = 0, e[2i] for q = 1;
 *   5. bit[i] = d[i] ^ d[i-1] over the stream, d[-1] = 0;
 *   6. code[i], i >= 25: the 26-bit word ending at bit i (first bit most significant), syndrome
 *      crc10(word >> 10) ^ (word & 0x3FF) with generator 0x5B9; 1..5 where it equals the offset word
 *      A 0x0FC, B 0x198, C 0x168, C' 0x350, D 0x1B4, else 0 (and 0 for i < 25).
 * A call takes whole windows: n_blocks a multiple of fmrx_rds_granule's blocks (24, 24, 3, 1 in
 * modes 0..3; with a capture rate set, the least common multiple with fmrx_wide_granule's), else
 * FMRX_EINVAL and nothing runs.  rds: the mixer rows as fmrx_rds_device returns them.  Outputs, each
 * may be NULL, per stream and W = windows of the call: bits and codes 76 W bytes each, win 2 W bytes
 * (p, q), y 2432 W floats (the 38 kS/s samples; for tests).  The state (resampler history, last sign,
 * chip and symbols) lives in the context beside the front half's, starts as above, is cleared by
 * fmrx_reset and is not part of the fmrx_get_state blob.                                          */
int fmrx_rds_granule(const fmrx_ctx* ctx, size_t* blocks);
int fmrx_rds_bits(fmrx_ctx* ctx, const float* rds, size_t n_blocks, uint8_t* bits, uint8_t* codes,
                  uint8_t* win, float* y);
int fmrx_rds_bits_device(fmrx_ctx* ctx, const float* d_rds, size_t n_blocks, uint8_t* d_bits,
                         uint8_t* d_codes, uint8_t* d_win, float* d_y);

#define FMRX_RDS_TAIL 103  /* bits the parser carries: a group is judged when its 104th bit arrives */
/* What the parser has read so far.  Plain data: copy it, compare it; fmrx_rds_info_init gives the
 * start (characters not yet received are spaces, ps and rt are NUL-terminated).                   */
typedef struct {
    uint64_t bits;      /* bits seen                                                               */
    uint64_t blocks;    /* of them, ends of a word with a valid offset word (code != 0)            */
    uint64_t groups;    /* groups accepted                                                         */
    uint16_t pi;        /* block A of the last group                                               */
    uint8_t pty, tp;    /* block B of the last group                                               */
    uint8_t rt_ab;      /* RadioText A/B flag of the last 2A/2B group                              */
    uint8_t tail_n;     /* the carried tail: the last min(bits, FMRX_RDS_TAIL) bits and codes      */
    char ps[9];
    char rt[65];
    uint8_t tail_bits[FMRX_RDS_TAIL];
    uint8_t tail_codes[FMRX_RDS_TAIL];
} fmrx_rds_info;
int fmrx_rds_info_init(fmrx_rds_info* io);
/* Host only, no context.  n bits and their codes (one byte each, as fmrx_rds_bits writes them) in
 * stream order, in pieces of any size: the result depends on the bits, not on how they were cut.
 * A group is accepted where codes A, B, C or C', D end 26 bits apart; no error correction.  Every
 * group sets pi, pty, tp; 0A/0B set two characters of ps at 2 (B & 3) from block D; 2A sets four of
 * rt at 4 (B & 15) from blocks C and D, 2B two at 2 (B & 15) from block D, and a change of the A/B
 * flag (B bit 4) first clears rt.  Bytes outside 0x20..0x7E are stored as spaces.                 */
int fmrx_rds_parse(fmrx_rds_info* io, const uint8_t* bits, const uint8_t* codes, size_t n);
/* Front half, bits and parse of n_blocks demod blocks (as fmrx_rf_block returns them; whole RDS
 * granules) into the context's per-stream info, which fmrx_rds_info_get copies out.              */
int fmrx_rds_decode(fmrx_ctx* ctx, const float* demod, size_t n_blocks);
int fmrx_rds_decode_device(fmrx_ctx* ctx, const float* d_demod, size_t n_blocks);
int fmrx_rds_info_get(const fmrx_ctx* ctx, int stream, fmrx_rds_info* out);
/* on != 0: the calls whose front end writes demod rows (tuned fmrx_process / _device / _device_ex,
 * fmrx_process_shared / _device, fmrx_process_wide / _device) also run fmrx_rds_decode_device on
 * those rows, on the same stream after the front end, and return after the parse (a host
 * synchronisation).  Such a call must be whole RDS granules (FMRX_EINVAL and nothing runs
 * otherwise).  The PCM is the same either way.  Off (the default): no call does anything more.    */
int fmrx_set_rds(fmrx_ctx* ctx, int on);

/* ---- RDS block sync: per-block acceptance, burst correction, block-wise groups ---- */
/* A stage behind fmrx_rds_bits' bits, off by default; signs and integers only.  Per stream, over the bits
 * b[0 .. N) it has been given since fmrx_reset:
 *   1. s[i], i >= 25: step 6's syndrome of the 26-bit word w[i] ending at bit i.
 *   2. The burst table (fmrx_rds_sync_design, host only): 1024 entries by syndrome, the 26-bit error pattern
 *      that is a burst of length <= B (first and last bit of the burst set) at some shift and has that
 *      syndrome, else FMRX_RDS_NO_BURST; entry 0 is the empty pattern.  B = 2: 51 patterns; no two bursts
 *      share a syndrome for B <= 5 (a collision would make the design fail with FMRX_ESTATE).
 *   3. Slots u = 0..3 are A, B, C*, D (C*: C or C').  With e = s[i] ^ offset word, w[i] is exact for the
 *      slot where e == 0 and correctable where the table holds a pattern for e; slot 2 tries exact C,
 *      exact C', correctable C, correctable C' in that order.  The information word is (w ^ pattern) >> 10.
 *   4. votes[u][i] = the j in -J .. J, j != 0, for which position i + 26 j is exact for slot (u + j) mod 4;
 *      positions in front of the stream's first word, and (at a flush) past its last bit, are no match.
 *   5. Position i carries a block of slot u if it is exact or correctable for u and votes[u][i] >= V; of
 *      several such slots the one with the most votes, the lowest u on a tie.
 * A position is judged once its 26 J bits of lookahead have arrived: a call judges those positions and the
 * context carries the last 25 + 52 J bits a stream, so any split of a stream into calls gives the same
 * records.  fmrx_rds_blocks_flush judges the positions still pending, the bits that have not arrived
 * counting as no match; bits given afterwards continue the same stream.  fmrx_reset clears the carry (and
 * the streams' fmrx_rds_ext) and keeps the switch; none of it is in the fmrx_get_state blob.              */
#define FMRX_RDS_NO_BURST 0xFFFFFFFFu
typedef struct { int J, V, B; } fmrx_rds_sync_config;   /* defaults 8, 3, 2; 1 <= J <= 8, 1 <= V <= 2 J, 0 <= B <= 5 */
int fmrx_rds_sync_config_default(fmrx_rds_sync_config* cfg);
int fmrx_rds_sync_design(int B, uint32_t* table /* 1024, may be NULL */, int* patterns /* may be NULL */);
/* An accepted block: the stream index of its last bit, the slot (0..3), whether C* matched as C', whether a
 * burst was corrected, the votes it had and its 16 information bits.  pad is zero.                        */
typedef struct { uint64_t bit; uint16_t info; uint8_t slot, c_prime, corrected, votes; uint8_t pad[2]; } fmrx_rds_block_rec;
/* The primitive.  bits: n_streams rows of n_bits bytes (bit 0 of each is used), any n_bits.  blocks:
 * n_streams rows of max_blocks records, a stream's accepted blocks in bit order; counts: n_streams, the
 * blocks accepted (where it exceeds max_blocks the row holds the first max_blocks); n_bits <= 2^30.  cfg =
 * NULL: the defaults; a cfg other than the one the stream began with is FMRX_EINVAL until fmrx_reset.  The device
 * form is asynchronous on the context stream and all its pointers are device memory.                     */
int fmrx_rds_blocks(fmrx_ctx* ctx, const fmrx_rds_sync_config* cfg, const uint8_t* bits, size_t n_bits,
                    fmrx_rds_block_rec* blocks, size_t max_blocks, uint32_t* counts);
int fmrx_rds_blocks_device(fmrx_ctx* ctx, const fmrx_rds_sync_config* cfg, const uint8_t* d_bits, size_t n_bits,
                           fmrx_rds_block_rec* d_blocks, size_t max_blocks, uint32_t* d_counts);
/* Host buffers; blocks and counts may both be NULL (at most 26 J positions a stream are pending).  With
 * fmrx_set_rds_sync on, the records also go into the streams' fmrx_rds_ext and close their open groups.    */
int fmrx_rds_blocks_flush(fmrx_ctx* ctx, fmrx_rds_block_rec* blocks, size_t max_blocks, uint32_t* counts);

#define FMRX_RDS_EXT_TAIL 16  /* records the block-wise parser keeps */
#define FMRX_RDS_MAX_AF 25
/* What the block-wise parser has read so far.  Plain data, as fmrx_rds_info is; fmrx_rds_ext_init gives the
 * start (characters not yet received are spaces; ps, rt and ptyn are NUL-terminated).                     */
typedef struct {
    uint64_t bits;              /* bits the records came from (the n_bits given)                           */
    uint64_t exact_blocks;      /* records without a correction                                            */
    uint64_t corrected_blocks;  /* records with one                                                        */
    uint64_t groups;            /* B blocks closed with A, C* and D all there                              */
    uint64_t partial_groups;    /* B blocks closed with one of them missing                                */
    uint16_t pi;                /* the last exact A block (valid where pi_set)                             */
    uint8_t pi_set;
    uint8_t pty, tp;            /* the last B block                                                        */
    uint8_t ta, ms, di;         /* the last group 0: TA, MS, and the four DI bits (d3 the most significant) */
    uint8_t rt_ab, ptyn_ab;     /* the A/B flags of the last group 2 and group 10A                         */
    uint8_t ps_sure, ptyn_sure; /* bit k: character k was written by blocks without a correction           */
    uint64_t rt_sure;
    uint8_t af_n;               /* AF codes kept (1..204: 87.5 MHz + 0.1 MHz x code), first appearance first */
    uint8_t af_count;           /* the last count a 0A group announced (code 224 + count)                  */
    uint8_t af[FMRX_RDS_MAX_AF];
    uint8_t ct_set;             /* a group 4A with B, C and D uncorrected has been read; its fields follow */
    uint8_t ct_hour, ct_minute, ct_month, ct_day;
    int8_t ct_offset;           /* local time offset in half hours                                         */
    uint16_t ct_year;           /* year, month, day of ct_mjd by IEC 62106 annex G in integers (good from
                                   1900-03-01 to 2100-02-28; zeros below MJD 15079)                        */
    uint32_t ct_mjd;
    char ps[9];
    char rt[65];
    char ptyn[9];
    uint8_t tail_n;             /* the carried tail: the last records, oldest first, and which B are closed */
    uint8_t tail_done[FMRX_RDS_EXT_TAIL];
    fmrx_rds_block_rec tail[FMRX_RDS_EXT_TAIL];
} fmrx_rds_ext;
int fmrx_rds_ext_init(fmrx_rds_ext* io);
/* Host only, no context.  n records of one stream in bit order, in pieces of any size (the result depends on
 * the records, not on how they were cut); n_bits is added to io->bits.  Every record is counted; an exact A
 * block sets pi.  A B block at bit i is closed, with whichever of the blocks at i - 26 (A), i + 26 (C*) and
 * i + 52 (D) are among the last FMRX_RDS_EXT_TAIL records, once a record at or past i + 52 has come, or at
 * flush != 0 (which closes every open one).  A corrected A block counts only if it equals pi.  B sets tp and
 * pty.  Group 0A/0B: TA, MS and the DI bit of segment B & 3; D gives two characters of ps; 0A with C, the AF
 * codes 1..204 (at most FMRX_RDS_MAX_AF, in order of first appearance) and the count 224..249.  Group 2A: C
 * gives two characters of rt at 4 (B & 15), D the next two; 2B: D two at 2 (B & 15); a change of the A/B flag
 * first clears rt, as in fmrx_rds_parse.  Group 4A with C and D: the clock time (hour < 24 and minute < 60,
 * else ignored).  Group 10A: ptyn at 4 (B & 1) as rt of 2A, with an A/B flag of its own.  A C' block never
 * supplies version-A contents.  Bytes outside 0x20..0x7E are stored as spaces; every other group type sets
 * tp and pty alone.
 * A correction can be wrong (a longer error that looks like a short burst), so corrected blocks count for
 * less: characters from a B and a C or D block both without a correction are always written and mark their
 * places (ps_sure, rt_sure, ptyn_sure); characters with a correction in either block are written only to
 * places not so marked.  A corrected B block may not change an A/B flag: where its flag differs, the group's
 * text is left out.  AF codes and the clock time, which nothing soon repeats, are taken only where B and the
 * blocks read are all without a correction.                                                              */
int fmrx_rds_parse_blocks(fmrx_rds_ext* io, const fmrx_rds_block_rec* blocks, size_t n, uint64_t n_bits, int flush);
/* on != 0: with fmrx_set_rds on too, every call that decodes RDS also runs the block sync (default
 * constants) over the bits it produces, on the same stream, copies the streams' counts and records back
 * and parses them into the streams' fmrx_rds_ext, which fmrx_rds_ext_get copies out.  The PCM and
 * fmrx_rds_info are the same either way.  With fmrx_set_rds off the stage does nothing.  Off (the default):
 * no call launches, allocates or copies anything more.                                                   */
int fmrx_set_rds_sync(fmrx_ctx* ctx, int on);
int fmrx_rds_ext_get(const fmrx_ctx* ctx, int stream, fmrx_rds_ext* out);

/* ---- arctan demodulator and PSD estimate (floating-point diagnostics) ------ */
/* fmDemodArctan: out[k] = atan2(Q,I) phase difference to the previous sample, wrapped into
 * [-pi, pi] as np.unwrap does; computed in double, stored as float.  d_prev_phase (one double,
 * in/out) is the phase before d_i[0]; on return the principal phase of the last sample (the
 * model returns the unwrapped one: equal mod 2 pi).  Device buffers, async.  d_out must be neither
 * d_i nor d_q; n = 0 leaves the phase as it was.                                               */
int fmrx_fm_demod_arctan(fmrx_ctx* ctx, float* d_out, double* d_prev_phase, const float* d_i,
                         const float* d_q, int n);
/* estimatePSD: Hann window, floor(n / freq_bins) segments, 10 log10(4/(Fs N) |X|^2) for the
 * freq_bins/2 positive bins, averaged in dB over segments.  freq_bins: power of two in
 * [2, 8192] (FFT in double; the reference's O(N^2) float DFT allows any N); n >= freq_bins.
 * Host buffers: freq and psd_db hold freq_bins/2 floats (freq[i] = i * fs / freq_bins).    */
int fmrx_estimate_psd(fmrx_ctx* ctx, const float* samples, size_t n, int freq_bins, float fs,
                      float* freq, float* psd_db);
int fmrx_psd_device(fmrx_ctx* ctx, const float* d_samples, size_t n, int freq_bins, float fs,
                    float* d_psd_db);

/* ---- deterministic synthetic FM-stereo IQ; identical bytes host/device ---- */
/* Stream `seed`, samples [first_pair, first_pair+n_pairs) of a stream at rf_fs.            */
int fmrx_synth_host(uint64_t seed, int rf_fs, uint64_t first_pair, size_t n_pairs, uint8_t* out);
int fmrx_synth_device(fmrx_ctx* ctx, uint64_t seed, int rf_fs, uint64_t first_pair,
                      size_t n_pairs, uint8_t* d_out);
/* n_seeds streams in ONE launch: stream k (seed seeds[k], host array) is written at
 * d_out + k * stride_bytes, samples [first_pair, first_pair + n_pairs) each (stride_bytes even
 * and >= 2 n_pairs).  Returns after the launch has completed (the seed table is uploaded).    */
int fmrx_synth_device_streams(fmrx_ctx* ctx, const uint64_t* seeds, size_t n_seeds, int rf_fs,
                              uint64_t first_pair, size_t n_pairs, uint8_t* d_out, size_t stride_bytes);

/* ---- test hook: the PLL's fallback libm (src/filter.cpp:161,168-170 on refused args) ---- */
/* Runs the device functions the PLL calls where its certified fast paths refuse, on device
 * buffers (context stream, async): kind 0 -> d_out[2i] = float(sin a_i), d_out[2i+1] =
 * float(cos a_i); kind 1 -> d_out[i] = float(atan2(a_i, b_i)); kind 2 -> d_out[i] = the NCO's
 * float(cos a_i).  tests/test_gpu_parity.py checks them against glibc's floats
 * (tests/golden/pll_fallback.npz).                                                         */
int fmrx_test_pll_fallback(fmrx_ctx* ctx, int kind, const float* d_a, const float* d_b, size_t n,
                           float* d_out);

/* ---- diagnostic: clock stamps of the fused mono kernel ---------------------------------- */
/* With d_stamps set, the mode-0 101-tap fused kernel (default variant) also writes, per     *
 * workgroup w, 6 u64 at d_stamps[6w..]: shader-clock counter at start and end, the 100 MHz  *
 * counter at start and end, HW_ID, XCC_ID (tools/mono_stamps.py: effective clock, wave       *
 * lifetimes, per-XCD balance).  Results are unchanged.  *needed = the largest grid a call    *
 * can launch (n_streams x 256 x resident workgroups per CU).  d_stamps = NULL turns it off. */
int fmrx_debug_mono_stamps(fmrx_ctx* ctx, unsigned long long* d_stamps, size_t n_workgroups, size_t* needed);

/* ---- diagnostic: speculative PLL counters ------------------------------------------------ */
/* With d_counts set (2 u64 on the device, zeroed and owned by the caller), every speculative  *
 * PLL segment of the stereo path and of fmrx_pll adds the runner's 16-step batches that did    *
 * not verify (resumed on the certified path) to d_counts[0] and the batches checked to         *
 * d_counts[1].  Results are unchanged.  d_counts = NULL turns it off.                          */
int fmrx_debug_pll_stats(fmrx_ctx* ctx, unsigned long long* d_counts);

/* ---- diagnostic: per-stream redos of the self-certifying PLL runners ----------------------- */
/* With d_counts set (n_streams x 8 u32 on the device, zeroed and owned by the caller), the stereo *
 * calls and fmrx_pll (as stream 0) add, per stream s and trigOffset range r of a runner launch    *
 * (r = 0 [2^17, 2^20), 1 [2^20, 2^21), 2 [2^21, 2^22), 3 from 2^22, the stuck 2^24 included):     *
 * d_counts[8 s + r] += the intervals the runner redid on the exact path (a trigArg outside its    *
 * candidates or an uncertified step), d_counts[8 s + 4 + r] += the steps it ran demoted (most of   *
 * its last 32 intervals missed, as on an unlocked loop: the rest of the range on the exact path). *
 * Demoted steps are filed under the range of the trigOffset at which the stream was demoted: in a *
 * call whose runner launches share one demoted launch (the pipelined engine, one a chunk), the    *
 * steps of the later launches it covers land in that slot too, also past a range boundary.  The   *
 * sum of a stream's slots 4 .. 7 is its demoted steps.                                            *
 * Results are unchanged.  d_counts = NULL turns it off.                                           */
int fmrx_debug_pll_redos(fmrx_ctx* ctx, unsigned* d_counts);

/* ---- diagnostic: per-stage device time of the stereo engine ------------------------------ */
/* op 1 arms (and clears) HIP event pairs around every stage launch of the following stereo     *
 * calls (ms of overlapping stages add up); op 0 reads, op -1 reads and disarms.  Stage k of     *
 * n_kinds: 0 RF front end, 1 band-pass pair, 2 PLL pre-pass, 3 lane runner, 4 two-wave          *
 * predicted runner, 5 saturated runner, 6/7/8 three-wave runner forms from trigOffset 2^20 /   *
 * 2^21 / 2^22, 9 check, 10 resume/tail, 11 NCO, 12 audio, 13/14/15 index runner forms from     *
 * trigOffset 2^17 / 2^18 / 2^19, 16-20 count runner forms from 2^17 / 2^18 / 2^19 / 2^20 /      *
 * 2^21 (FMRX_KNOB_PLL_CNT), 21 the three-candidate stick form (trigOffset stuck at 2^24).      *
 * ms[k] = summed device time,                                                                    *
 * launches[k] = launches, steps[k] = serial PLL steps a runner kind ran as its segment's only  *
 * runner (per stream chain; for ns per step of each regime).  Results are unchanged.           */
int fmrx_debug_stage_timing(fmrx_ctx* ctx, int op, double* ms, double* steps, long* launches, int n_kinds);

/* ---- diagnostic / test knobs of one context ----------------------------------------------- */
/* None of them changes the output.  The tuning knobs pick which kernel form runs (A/B
 * measurements); a new context takes them from the environment variable named beside each
 * (read once, at fmrx_create).  The PLL test hooks make the runners do extra work that their
 * exact paths then redo (bit-identical output, counted by fmrx_debug_pll_stats); they are set
 * only here, never from the environment.  value: the knob's integer (the skew: samples).
 * Accepted range [lo, hi] in brackets: fmrx_debug_set_knob returns FMRX_EINVAL for a value
 * outside it (or a fraction for an integer knob), fmrx_create for such an environment variable
 * (tests/test_gpu_parity.py test_knob_sweep_bit_exact sweeps every value of every range).      */
#define FMRX_KNOB_PLL_SPEC 0          /* [0,1] 1 speculative runners, 0 the certified launch FMRX_PLL_SPEC */
#define FMRX_KNOB_PLL_SAT 1           /* [0,1] 0: no saturated-segment runner            FMRX_PLL_SAT  */
#define FMRX_KNOB_PLL_PRED 2          /* [0,2] 0 no predicted runners, 2 forced on       FMRX_PLL_PRED */
#define FMRX_KNOB_PLL_PIPE 3          /* [0,1] 0: no three-wave runner                   FMRX_PLL_PIPE */
#define FMRX_KNOB_PLL_IDX 4           /* [0,2] 2 index runner from 2^17, 1 from 2^18, 0 off FMRX_PLL_IDX */
#define FMRX_KNOB_STEREO_CHUNKS 5     /* [0,64] 0 auto, k chunks (1 the serial engine)  FMRX_STEREO_CHUNKS */
#define FMRX_KNOB_MONO_SPLIT 6        /* [-1,1023] -1 default, 0 equal, n/1024 older wave's FMRX_MONO_SPLIT */
#define FMRX_KNOB_BPF_TILE 7          /* [0,1] 0: the per-output band-pass kernel        FMRX_BPF_TILE */
#define FMRX_KNOB_HALO_KERNEL 8       /* [0,1] 1: the separate halo kernel            FMRX_HALO_KERNEL */
#define FMRX_KNOB_PLL_INJECT 9        /* [-1,2^30] test hook: runners corrupt batch 1+(k+s)%(nb-1) of stream s */
#define FMRX_KNOB_PLL_PIPE_MISS 10    /* [-2^30,2^30] test hook: self-certifying runners miss interval k
                                         (k >= 1), every interval from -k - 1 on (k <= -2: the demotion
                                         runs), none (-1, 0)                                            */
#define FMRX_KNOB_PLL_HINT_SKEW 11    /* [-2^24,2^24] test hook: host trigOffset bounds shifted by value */
#define FMRX_KNOB_PLL_CNT 12          /* [0,31] bit f-17: count runner for form f's range (12) FMRX_PLL_CNT */
#define FMRX_KNOB_PLL_STICK 13        /* [0,1] 1: the stick form past trigOffset 2^24    FMRX_PLL_STICK */
#define FMRX_KNOB_STEREO_HEAD 14      /* [1,64] first chunk in 16ths of a chunk (8)    FMRX_STEREO_HEAD */
#define FMRX_KNOB_STEREO_LEAD 15      /* [0,64] n: chunk k's front end after chunk k-n's PLL FMRX_STEREO_LEAD */
#define FMRX_KNOB_AUDIO_DEFER 16      /* [0,64] 0 beside the next PLL, 1 after the last, 2 (default) all but
                                         the last chunk's beside the last PLL, 2 + e: the first e of those
                                         beside the PLL before it (e past the chunks: all of them)
                                                                                     FMRX_AUDIO_DEFER */
#define FMRX_KNOB_STEREO_TAIL 17      /* [1,64] last chunk in 16ths of a chunk (8)     FMRX_STEREO_TAIL */
int fmrx_debug_set_knob(fmrx_ctx* ctx, int knob, double value);

#ifdef __cplusplus
}
#endif
#endif /* FMRX_H */
