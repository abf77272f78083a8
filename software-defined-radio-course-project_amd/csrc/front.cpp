// front.cpp — the front ends ahead of the audio stages other than the fused kernel: the tuned front
// end (tuner.hip) and the capture stage in front of it (wide.h: one host path around wide.hip for an
// integer ratio and rate.hip for a rational one), with the calls that configure them: tuning, the raw
// I/Q format, the capture decimation and the capture rate.
#include "ctx.h"

#include <numeric>

using namespace fmrx;

namespace {

// One launch of the tuner kernel over n_blocks blocks a stream: source rows of `format` (iq_stride
// bytes apart, 0 for a shared capture), the halo pair `halo` of halo_bytes a stream, its current one
// in front of the call, demod rows out.  Flips the pair and advances the position.
int launch_front(fmrx_ctx* c, const uint8_t* d_iq, size_t iq_stride, int format, PingPong<uint8_t>& halo, size_t halo_bytes, size_t n_blocks, float* d_demod, size_t demod_stride, int demod_hist,
                 bool pre_tail) {
    const int ns = c->cfg.n_streams;
    TunerLaunch L{};
    L.iq = d_iq;
    L.iq_stride = iq_stride;
    L.halo = halo.cur();
    L.halo_next = halo.next();
    L.halo_bytes = halo_bytes;
    L.stream_bytes = n_blocks * c->geo.iq_pairs * (size_t)iq_pair_bytes(format);
    L.format = format;
    L.demod = d_demod;
    L.demod_stride = demod_stride;
    L.demod_hist = demod_hist;
    L.pre_tail = pre_tail ? 1 : 0;
    L.n_if = (long long)(n_blocks * c->geo.if_samples);
    L.segs = tuner_segments(L.n_if, c->geo.rf_taps, c->geo.rf_decim, ns, c->n_simd / 4, c->tune.max_n);
    L.streams = reinterpret_cast<const TunerStream*>(c->tune.streams.p);
    L.tables = reinterpret_cast<const float2*>(c->tune.tab.p);
    L.first_pair = c->tune.pos;
    const int st_t = c->diag.timer.begin(c->stream);
    const int rc = launch_tuner(L, ns, c->geo.rf_taps, c->geo.rf_decim, c->tune.max_n, c->taps.mono, c->stream);
    c->diag.timer.end(st_t, kStFront, 0.0, c->stream);
    if (rc != 0) return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "tuned front end launch failed (%d)", rc);
    halo.flip();
    c->tune.pos += (uint64_t)n_blocks * c->geo.iq_pairs;
    return 0;
}

}  // namespace

namespace fmrx {

int init_front(fmrx_ctx* c) {
    const size_t ns = c->cfg.n_streams;
    c->front.halo_bytes = mono_halo_bytes(c->geo.rf_taps, c->geo.rf_decim, c->geo.audio_down);
    c->front.halo_pairs = c->front.halo_bytes / 2;
    c->tune.offsets.assign(ns, 0);
    c->wide.offsets.assign(ns, 0);
    return c->front.halo.ensure(c->front.halo_bytes * ns);
}

// The halo filled with the format's zero; the position back to 0, the offsets stay (configuration)
int reset_front(fmrx_ctx* c) {
    PingPong<uint8_t>& h = c->front.halo;
    c->tune.pos = 0;
    for (auto& b : h.buf) HIPCHK(hipMemsetAsync(b.p, iq_zero_byte(c), c->front.halo_bytes * c->cfg.n_streams, c->stream));
    h.rewind();
    return 0;
}

// The wide stage: history of the format's zero, narrow halo of 0.0f
int reset_wide(fmrx_ctx* c) {
    auto& w = c->wide;
    if (!w.ratio.on()) return 0;
    HIPCHK(hipMemsetAsync(w.hist.p, iq_zero_byte(c), w.ratio.hist_pairs() * c->front.pair_bytes, c->stream));
    for (auto& b : w.halo.buf) HIPCHK(hipMemsetAsync(b.p, 0, c->front.halo_pairs * 8 * c->cfg.n_streams, c->stream));
    w.halo.rewind();
    return 0;
}

// The tuned front end over n_blocks blocks a stream of the context's format: demod rows out, the
// halo moved, the position advanced.  iq_stride: bytes between the streams' rows, 0 for a shared
// capture.  pre_tail: also the 50 demod samples in front of the call (at demod_hist - 50, from the
// halo).
int run_tuned_front(fmrx_ctx* c, const uint8_t* d_iq, size_t iq_stride, size_t n_blocks, float* d_demod,
                    size_t demod_stride, int demod_hist, bool pre_tail) {
    const size_t unit = 2 * c->front.pair_bytes;  // the kernel's staging unit: two pairs
    if (reinterpret_cast<uintptr_t>(d_iq) % unit != 0 || iq_stride % unit != 0)
        return fail(FMRX_EINVAL, "tuned calls need %zu-byte aligned I/Q rows", unit);
    int rc_size = check_call_size(c, n_blocks);
    if (rc_size) return rc_size;
    return launch_front(c, d_iq, iq_stride, c->front.format, c->front.halo, c->front.halo_bytes, n_blocks, d_demod,
                        demod_stride, demod_hist, pre_tail);
}

// The taps on the demod rows, the meter (fmrx_set_meter), soft stereo's levels (fmrx_set_stereo_blend),
// quieting's levels (fmrx_set_quieting), the RDS decode (fmrx_set_rds) and the carrier sums (fmrx_set_afc), in that order everywhere; a further tap
// is one line in each of the three.
// check_taps: the call is whole granules of every tap that is on (the RDS decode's refusal first).  The
// levels read the meter's powers: one meter launch serves both, and only fmrx_set_meter has them copied
// back and added to its reports.  The carrier sums' finish comes last: with tracking it may retune.
static int check_taps(const fmrx_ctx* c, size_t n_blocks) {
    int rc = c->rdsb.on ? check_rds_blocks(c, n_blocks) : 0;
    if (!rc && c->meter.on) rc = check_frame_blocks(c, n_blocks, "a meter call");
    if (!rc && c->afc.on) rc = check_frame_blocks(c, n_blocks, "a carrier call");
    if (!rc && blend_metered(c)) rc = check_frame_blocks(c, n_blocks, "a call with soft stereo on");
    return rc || !quiet_metered(c) ? rc : check_frame_blocks(c, n_blocks, "a call with quieting on");
}
// a stage's level follower over the call's frames: from the powers the meter kernel leaves in meter.pow for
// this call, or under hold the streams' last levels over the meter frames the call's audio frames reach
static int levels_of_call(fmrx_ctx* c, LevelFollower& F, const float* d_thr, size_t n_blocks) {
    const size_t ns = c->cfg.n_streams, frames = meter_frames(c, n_blocks), na = n_blocks * c->geo.audio_frames;
    if (F.hold) return levels_enqueue_held(F, c->stream, ns, (na * c->frames.Gm + c->frames.A - 1) / c->frames.A);
    F.pending = 0;
    if (frames < 1 || frames > 0x7FFFFFFFull / kMeterTones) return fail(FMRX_EINVAL, "%zu blocks: too many frames for one call", n_blocks);
    return levels_enqueue(F, c->stream, ns, c->meter.pow.p, d_thr, frames);
}
static int taps_enqueue(fmrx_ctx* c, size_t n_blocks) {
    const float* rows = c->stereo.demod.p + kDemodHist;
    int rc = c->meter.on || blend_metered(c) || quiet_metered(c) ? meter_enqueue(c, rows, c->stereo.demod_stride, n_blocks) : 0;
    if (!rc && c->blend.on) rc = levels_of_call(c, c->blend.f, c->blend.thr.p, n_blocks);
    if (!rc && c->quiet.on) rc = levels_of_call(c, c->quiet.f, c->quiet.tab.p, n_blocks);
    if (!rc && c->rdsb.on) rc = rds_decode_enqueue(c, rows, c->stereo.demod_stride, n_blocks);
    return rc || !c->afc.on ? rc : afc_enqueue(c, rows, c->stereo.demod_stride, n_blocks);
}
static int taps_finish(fmrx_ctx* c) {
    int rc = c->meter.on ? meter_finish(c) : 0;
    if (!c->meter.on) c->meter.pending = 0;  // powers soft stereo or quieting alone asked for: nothing to report
    if (!rc && c->blend.on) rc = blend_finish(c);
    if (!rc && c->quiet.on) rc = quiet_finish(c);
    if (!rc && c->rdsb.on) rc = rds_decode_finish(c);
    return rc || !c->afc.on ? rc : afc_finish(c);
}

// The audio stage of a call whose front end filled the context's demod rows (mono: the polyphase
// stage; stereo: the non-pipelined engine).  The taps read the same rows on the stream in front of it
// (the audio stage moves the rows' tail afterwards) and are parsed and added once the call's work is
// done; the audio stage reads and writes nothing they touch.
static int run_audio_stage(fmrx_ctx* c, size_t n_blocks, int16_t* d_pcm, float* d_mono) {
    const size_t n_if = n_blocks * c->geo.if_samples;
    int rc = taps_enqueue(c, n_blocks);
    if (rc) return rc;
    if (c->cfg.channels != FMRX_MONO)
        rc = run_stereo_audio(c, n_blocks, d_pcm, d_mono);
    else
        rc = run_mono_audio(c, c->stereo.demod.p + kDemodHist, c->stereo.demod_stride, n_if, d_pcm, d_mono);
    return rc ? rc : taps_finish(c);
}

// A tuned call: the front end for the whole call into the context's demod rows, then the audio
// stage fmrx_audio_block runs (mono: the polyphase stage; stereo: the non-pipelined engine).
int run_tuned(fmrx_ctx* c, const uint8_t* d_iq, size_t iq_stride, size_t n_blocks, int16_t* d_pcm, float* d_mono) {
    const int ns = c->cfg.n_streams;
    const size_t n_if = n_blocks * c->geo.if_samples;
    int rc = check_taps(c, n_blocks);
    if (rc || (rc = ensure_demod(c, n_if))) return rc;
    if (c->cfg.channels != FMRX_MONO) {
        if ((rc = run_tuned_front(c, d_iq, iq_stride, n_blocks, c->stereo.demod.p, c->stereo.demod_stride, kDemodHist, false)))
            return rc;
        return run_audio_stage(c, n_blocks, d_pcm, d_mono);
    }
    // after fmrx_seek the audio history is rebuilt from the halo, as the fused kernel's pre-roll
    // does: the 50 demod samples in front of the call (all a resampler output reads back)
    const bool stale = c->mono.stale;
    if ((rc = run_tuned_front(c, d_iq, iq_stride, n_blocks, c->stereo.demod.p, c->stereo.demod_stride, kDemodHist, stale)))
        return rc;
    if (stale) {
        if (launch_copy_streams(c->mono.hist.p + (c->mono.hist_len - kAudioHist50), c->mono.hist_len,
                                c->stereo.demod.p + (kDemodHist - kAudioHist50), c->stereo.demod_stride, kAudioHist50, ns,
                                c->stream))
            return fail(FMRX_EHIP, "audio history copy failed");
        c->mono.stale = false;
    }
    return run_audio_stage(c, n_blocks, d_pcm, d_mono);
}

}  // namespace fmrx

namespace {

// The streams' rotators for offsets_hz on the device (tables, TunerStream rows, tune_max_n);
// FMRX_EINVAL with nothing changed for an offset fmrx_tuner_design refuses.
int tuner_upload(fmrx_ctx* c, const int32_t* offsets_hz) {
    if (!tuner_supported(c->geo.rf_taps, c->geo.rf_decim))
        return fail(FMRX_EINVAL, "no tuned RF kernel for rf_taps=%d rf_decim=%d", c->geo.rf_taps, c->geo.rf_decim);
    int rc = set_device(c);
    if (rc) return rc;
    const size_t ns = c->cfg.n_streams;
    std::vector<TunerStream> ts(ns);
    size_t entries = 0;
    int max_n = 1;
    for (size_t s = 0; s < ns; s++) {  // every offset checked before anything changes
        int N = 0, k = 0;
        if ((rc = fmrx_tuner_design(c->geo.rf_fs, offsets_hz[s], &N, &k, nullptr))) return rc;
        ts[s] = TunerStream{(uint32_t)N, (uint32_t)k, (uint32_t)entries, 0u};
        entries += (size_t)N;
        max_n = std::max(max_n, N);
    }
    std::vector<float> tab(2 * entries);
    for (size_t s = 0; s < ns; s++) tuner_design(c->geo.rf_fs, offsets_hz[s], nullptr, nullptr, tab.data() + 2 * ts[s].tab);
    // a call in flight may still read the old tables: drain the stream before they are replaced
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((rc = c->tune.tab.ensure(tab.size())) || (rc = c->tune.streams.ensure(4 * ns))) return rc;
    HIPCHK(hipMemcpy(c->tune.tab.p, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->tune.streams.p, ts.data(), sizeof(TunerStream) * ns, hipMemcpyHostToDevice));
    c->tune.max_n = max_n;
    return FMRX_OK;
}

// The tables of offset 0 for every stream: what the untuned calls of a format other than u8 run with
// (no untuned kernel reads such a format: the tuned one at offset 0 gives the untuned bits)
int upload_zero_offsets(fmrx_ctx* c) {
    const std::vector<int32_t> zeros((size_t)c->cfg.n_streams, 0);
    return tuner_upload(c, zeros.data());
}

// y rows of one internal piece of a wide call: at most this many bytes over all streams (a piece
// is a whole number of granules, at least one)
constexpr size_t kWidePieceBytes = (size_t)128 << 20;

}  // namespace

namespace fmrx {

int check_capture_decim(int decim, bool or_one) {
    if ((decim >= kWideMinDecim && decim <= kWideMaxDecim) || (or_one && decim == 1)) return 0;
    return fail(FMRX_EINVAL, "capture decimation %d outside %d..%d", decim, or_one ? 1 : kWideMinDecim, kWideMaxDecim);
}

int check_wide_rf_fs(int rf_fs) {
    if (rf_fs <= 0 || rf_fs % 4 != 0) return fail(FMRX_EINVAL, "rf_fs %d is not a positive multiple of 4", rf_fs);
    return 0;
}

int check_wide_blocks(const fmrx_ctx* c, size_t n_blocks) {
    if (n_blocks % c->wide.ratio.blocks != 0)  // an integer ratio's granule is one block
        return fail(FMRX_EINVAL, "%zu blocks: a call at %d S/s takes whole granules of %zu blocks", n_blocks,
                    c->wide.ratio.cap_fs(c->geo.rf_fs), c->wide.ratio.blocks);
    return 0;
}

// A wide call (fmrx_process_wide_device; arguments checked, device set): per piece of whole granules
// the down-converter (wide.hip or rate.hip, by the ratio) into the y rows, then the tuned front end
// reading them as an f32 stream with the wide stage's own halo; the demod rows of the whole call then
// take the audio stage a tuned call takes.  A piece past the first finds its history in the capture itself.
int run_wide(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm) {
    const CaptureRatio& r = c->wide.ratio;
    const int ns = c->cfg.n_streams;
    const size_t ip = c->geo.iq_pairs, n_if = n_blocks * c->geo.if_samples, gran = r.blocks;
    const size_t hb = r.hist_pairs() * c->front.pair_bytes;
    int rc = check_taps(c, n_blocks);
    if (rc || (rc = ensure_demod(c, n_if))) return rc;
    const size_t fit = kWidePieceBytes / ((size_t)ns * ip * 8);
    const size_t piece = std::min(n_blocks, std::max(gran, fit / gran * gran));
    if (piece * ip * 2 > c->wide.y_stride) {  // grown on demand; a call in flight still reads the old rows
        HIPCHK(hipStreamSynchronize(c->stream));
        c->wide.y_stride = 0;
        if ((rc = c->wide.y.ensure((size_t)ns * piece * ip * 2))) return rc;
        c->wide.y_stride = piece * ip * 2;
    }
    const size_t nhb = c->front.halo_pairs * 8;
    for (size_t b0 = 0; b0 < n_blocks; b0 += piece) {
        const size_t nb = std::min(piece, n_blocks - b0);
        DdcLaunch L{};
        L.iq = d_iq + wide_pairs_of(c, b0) * c->front.pair_bytes;
        L.hist = b0 == 0 ? c->wide.hist.p : L.iq - hb;
        L.stream_bytes = wide_pairs_of(c, nb) * c->front.pair_bytes;
        L.y = c->wide.y.p;
        L.y_stride = c->wide.y_stride;
        L.n_out = (long long)(nb * ip);
        L.segs = wide_segments(L.n_out, r.up, r.down, ns, c->n_simd / 4);
        L.format = c->front.format;
        L.up = r.up;
        L.down = r.down;
        L.streams = reinterpret_cast<const WideStream*>(c->wide.streams.p);
        L.tables = reinterpret_cast<const float2*>(c->wide.tab.p);
        L.taps = c->wide.taps.p;
        L.first_pair = c->tune.pos / (uint64_t)r.up * (uint64_t)r.down;  // tune_pos is a multiple of up
        TimingPair* ev = nullptr;  // fmrx_kernel_timing: the down-converter's launches
        if ((rc = timing_begin(c, c->stream, &ev))) return rc;
        rc = launch_wide_ddc(L, ns, c->stream);
        if (rc != 0)
            return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "%sdown-converter launch failed (%d)", r.rational() ? "rational " : "", rc);
        if ((rc = timing_end(ev, c->stream))) return rc;
        // the y rows as an f32 stream, the wide stage's own halo in front of them
        if ((rc = launch_front(c, reinterpret_cast<const uint8_t*>(c->wide.y.p), c->wide.y_stride * sizeof(float), kIqF32,
                               c->wide.halo, nhb, nb, c->stereo.demod.p + b0 * c->geo.if_samples,
                               c->stereo.demod_stride, kDemodHist, false)))
            return rc;
    }
    // the next call's history: the capture's last raw pairs (a granule holds more than that)
    HIPCHK(hipMemcpyAsync(c->wide.hist.p, d_iq + wide_pairs_of(c, n_blocks) * c->front.pair_bytes - hb, hb,
                          hipMemcpyDeviceToDevice, c->stream));
    return run_audio_stage(c, n_blocks, d_pcm, nullptr);
}

}  // namespace fmrx

namespace {

// What fmrx_wide_design and fmrx_rate_design do once the ratio is known and within the limits: the split,
// the fine part to the tuner, and the outputs, written only on success.  kOffsetOutside (no error text
// set: the two word it differently) for 2 |offset| >= cap_fs.
constexpr int kOffsetOutside = 1;
int design_offset(int rf_fs, int up, int down, int offset_hz, int* coarse_hz, int* fine_hz, int* N, int* k, float* cos_sin,
                  int* taps, float* h) {
    int fc = 0, fr = 0, n = 0, kk = 0;
    if (!rate_split(rf_fs, up, down, offset_hz, &fc, &fr, &n, &kk, nullptr)) return kOffsetOutside;
    int tn = 0, tk = 0, rc;
    if ((rc = fmrx_tuner_design(rf_fs, fr, &tn, &tk, nullptr))) return rc;  // the fine part goes to the tuner
    if (coarse_hz) *coarse_hz = fc;
    if (fine_hz) *fine_hz = fr;
    if (N) *N = n;
    if (k) *k = kk;
    if (cos_sin) rate_split(rf_fs, up, down, offset_hz, nullptr, nullptr, nullptr, nullptr, cos_sin);
    if (taps) *taps = rate_taps(down);
    if (h) design_lpf(h, (float)rf_fs * (float)down, (float)(3.0 * rf_fs / 8.0), rate_taps(down), up);
    return FMRX_OK;
}

// The capture stage of the ratio up / down (`blocks` a granule) in place of the context's: the stream
// drained, the stage's buffers grown and its low-pass uploaded (none at 1/1), the ratio recorded, the
// state reset.  The ratio is the caller's to check.
int set_capture_stage(fmrx_ctx* c, int up, int down, size_t blocks) {
    int rc = set_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));  // a call in flight still reads the wide state
    if (down != up) {
        const size_t ns = c->cfg.n_streams;
        std::vector<float> h((size_t)rate_taps(down));
        design_lpf(h.data(), (float)c->geo.rf_fs * (float)down, (float)(3.0 * c->geo.rf_fs / 8.0), rate_taps(down), up);
        // the integer kernel reads the taps as they are, the rational one regrouped by phase
        std::vector<RateTap> hp(up == 1 ? 0 : (size_t)up * rate_phase_stride(up, down));
        if (up != 1) rate_taps_by_phase(h.data(), up, down, hp.data());
        const void* taps = up == 1 ? (const void*)h.data() : (const void*)hp.data();
        const size_t tap_floats = up == 1 ? h.size() : 2 * hp.size();
        if ((rc = c->wide.hist.ensure((size_t)rate_hist_pairs(up, down) * c->front.pair_bytes)) || (rc = c->wide.taps.ensure(tap_floats)) ||
            (rc = c->wide.tab.ensure(2 * (size_t)kRateMaxN * ns)) || (rc = c->wide.streams.ensure(2 * ns)) ||
            (rc = c->wide.halo.ensure(c->front.halo_pairs * 8 * ns)))
            return rc;
        HIPCHK(hipMemcpy(c->wide.taps.p, taps, sizeof(float) * tap_floats, hipMemcpyHostToDevice));
    }
    c->wide.ratio = CaptureRatio{up, down, blocks};
    c->wide.tuned = false;  // offsets are against cap_fs: fmrx_tune_wide again
    return reset_state(c);
}

}  // namespace

namespace fmrx {

// The streams' rotators for offsets_hz in place of the current ones, the position set, tuning on
int tune_narrow(fmrx_ctx* c, const int32_t* offsets_hz, uint64_t first_pair) {
    const int rc = tuner_upload(c, offsets_hz);
    if (rc) return rc;
    c->tune.offsets.assign(offsets_hz, offsets_hz + c->cfg.n_streams);
    c->tune.pos = first_pair;
    c->tune.on = true;
    c->wide.tuned = false;  // the tables are no longer the fine offsets of fmrx_tune_wide
    return FMRX_OK;
}

// The same on a context with a capture stage: every offset split into its coarse and fine part (first_pair
// a multiple of the ratio's down, in wide pairs)
int tune_wide(fmrx_ctx* c, const int32_t* offsets_hz, uint64_t first_pair) {
    const CaptureRatio& r = c->wide.ratio;
    const size_t ns = c->cfg.n_streams;
    std::vector<int32_t> fine(ns);
    std::vector<WideStream> ws(ns);
    std::vector<float> tab(2 * (size_t)kRateMaxN * ns, 0.0f);
    int rc;
    for (size_t s = 0; s < ns; s++) {  // every offset checked before anything changes
        int fr = 0, n = 0, k = 0;
        if ((rc = fmrx_rate_design(c->geo.rf_fs, r.cap_fs(c->geo.rf_fs), offsets_hz[s], nullptr, nullptr, nullptr, &fr, &n, &k,
                                   tab.data() + 2 * kRateMaxN * s, nullptr, nullptr)))
            return rc;
        fine[s] = fr;
        ws[s] = WideStream{(uint32_t)n, (uint32_t)k};
    }
    if ((rc = tuner_upload(c, fine.data()))) return rc;  // drains the stream before the tables change
    HIPCHK(hipMemcpy(c->wide.tab.p, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->wide.streams.p, ws.data(), sizeof(WideStream) * ns, hipMemcpyHostToDevice));
    c->tune.offsets = fine;  // the existing tuner state: the fine parts at rf_fs
    c->tune.pos = first_pair / (uint64_t)r.down * (uint64_t)r.up;
    c->tune.on = true;
    c->wide.offsets.assign(offsets_hz, offsets_hz + ns);
    c->wide.tuned = true;
    return FMRX_OK;
}

}  // namespace fmrx

extern "C" {

// ---- off-centre tuning ----------------------------------------------------------------------
int fmrx_tuner_design(int rf_fs, int offset_hz, int* N, int* k, float* cos_sin) {
    int why = 0;
    if (tuner_design(rf_fs, offset_hz, N, k, cos_sin, &why)) return FMRX_OK;
    if (why == 2)
        return fail(FMRX_EINVAL, "offset %d Hz at %d S/s: rotator period above %d pairs (use a multiple of 1 kHz)",
                    offset_hz, rf_fs, kTunerMaxN);
    return fail(FMRX_EINVAL, "offset %d Hz outside (-%d/2, %d/2)", offset_hz, rf_fs, rf_fs);
}

int fmrx_tune(fmrx_ctx* c, const int32_t* offsets_hz, uint64_t first_pair) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (!offsets_hz) {  // tuning off: the untuned kernels, exactly as before
        if (c->front.format != kIqU8) {
            const int rc = upload_zero_offsets(c);
            if (rc) return rc;
        }
        c->tune.on = false;
        c->wide.tuned = false;
        c->tune.pos = first_pair;
        afc_caller_tuned(c);
        return FMRX_OK;
    }
    const int rc = tune_narrow(c, offsets_hz, first_pair);
    if (!rc) afc_caller_tuned(c);
    return rc;
}

// ---- raw I/Q formats ----------------------------------------------------------------------------
int fmrx_iq_pair_bytes(int format) {
    const int b = iq_pair_bytes(format);
    return b > 0 ? b : fail(FMRX_EINVAL, "unknown I/Q format %d", format);
}

int fmrx_set_input_format(fmrx_ctx* c, int format) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    const int pb = iq_pair_bytes(format);
    if (pb < 0) return fail(FMRX_EINVAL, "unknown I/Q format %d", format);
    if (format != kIqU8 && !tuner_supported(c->geo.rf_taps, c->geo.rf_decim))
        return fail(FMRX_EINVAL, "no tuned RF kernel for rf_taps=%d rf_decim=%d: u8 input only", c->geo.rf_taps,
                    c->geo.rf_decim);
    int rc = set_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));  // a call in flight still reads the halo
    if (format != c->front.format) {
        const size_t ns = c->cfg.n_streams, hb = c->front.halo_pairs * (size_t)pb;
        if (format != kIqU8 && !c->tune.on && (rc = upload_zero_offsets(c))) return rc;
        if ((rc = c->front.halo.ensure(hb * ns))) return rc;
        if (c->wide.ratio.on() && (rc = c->wide.hist.ensure(c->wide.ratio.hist_pairs() * (size_t)pb))) return rc;
        c->front.format = format;
        c->front.pair_bytes = (size_t)pb;
        c->front.halo_bytes = hb;
    }
    return reset_state(c);
}

int fmrx_input_format(const fmrx_ctx* c, int* format) {
    CtxLock lock_(c);
    if (!c || !format) return fail(FMRX_EINVAL, "null argument");
    *format = c->front.format;
    return FMRX_OK;
}

int fmrx_tuner_info(fmrx_ctx* c, int32_t* offsets_hz, uint64_t* next_pair, int* enabled) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (offsets_hz) std::copy(c->tune.offsets.begin(), c->tune.offsets.end(), offsets_hz);
    if (next_pair) *next_pair = c->tune.pos;
    if (enabled) *enabled = c->tune.on ? 1 : 0;
    return FMRX_OK;
}

// ---- wide captures: the capture stage ahead of the tuner (an integer or a rational ratio) -----------
int fmrx_wide_design(int rf_fs, int decim, int offset_hz, int* coarse_hz, int* fine_hz, int* N, int* k, float* cos_sin,
                     int* taps, float* h) {
    int rc = check_capture_decim(decim, false);
    if (rc || (rc = check_wide_rf_fs(rf_fs))) return rc;
    rc = design_offset(rf_fs, 1, decim, offset_hz, coarse_hz, fine_hz, N, k, cos_sin, taps, h);
    if (rc == kOffsetOutside)
        return fail(FMRX_EINVAL, "offset %d Hz outside (-%d %d/2, %d %d/2)", offset_hz, decim, rf_fs, decim, rf_fs);
    return rc;
}

int fmrx_rate_design(int rf_fs, int cap_fs, int offset_hz, int* up, int* down, int* coarse_hz, int* fine_hz, int* N, int* k,
                     float* cos_sin, int* taps, float* h) {
    int l = 0, m = 0;
    const int kind = rate_ratio(rf_fs, cap_fs, &l, &m);
    if (kind < 0 || (kind == 1 && m == 1))
        return fail(FMRX_EINVAL, "capture rate %d S/s against %d S/s: need cap_fs / rf_fs = M / L with L <= %d, L < M <= %d, M <= 10 L",
                    cap_fs, rf_fs, kRateMaxUp, kRateMaxDown);
    // an integer ratio: fmrx_wide_design's range of the decimation and its wording of a refusal
    int rc = kind == 1 ? fmrx_wide_design(rf_fs, m, offset_hz, coarse_hz, fine_hz, N, k, cos_sin, taps, h)
                       : design_offset(rf_fs, l, m, offset_hz, coarse_hz, fine_hz, N, k, cos_sin, taps, h);
    if (rc == kOffsetOutside) rc = fail(FMRX_EINVAL, "offset %d Hz outside (-%d/2, %d/2)", offset_hz, cap_fs, cap_fs);
    if (rc) return rc;
    if (up) *up = l;
    if (down) *down = m;
    return FMRX_OK;
}

int fmrx_set_capture_decim(fmrx_ctx* c, int decim) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    const int rc = check_capture_decim(decim, true);
    if (rc) return rc;
    if (decim == 1 && !c->wide.ratio.on()) return FMRX_OK;  // the default: nothing anywhere changes
    if (decim > 1 && !tuner_supported(c->geo.rf_taps, c->geo.rf_decim))
        return fail(FMRX_EINVAL, "no tuned RF kernel for rf_taps=%d rf_decim=%d: no wide captures", c->geo.rf_taps,
                    c->geo.rf_decim);
    return set_capture_stage(c, 1, decim, 1);
}

int fmrx_set_capture_rate(fmrx_ctx* c, int cap_fs) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    int up = 0, down = 0;
    const int kind = rate_ratio(c->geo.rf_fs, cap_fs, &up, &down);
    if (kind < 0)
        return fail(FMRX_EINVAL, "capture rate %d S/s against %d S/s: need cap_fs / rf_fs = M / L with L <= %d, L < M <= %d, M <= 10 L",
                    cap_fs, c->geo.rf_fs, kRateMaxUp, kRateMaxDown);
    if (kind == 1) return fmrx_set_capture_decim(c, down);  // an integer ratio: its range of the decimation
    if (!tuner_supported(c->geo.rf_taps, c->geo.rf_decim))
        return fail(FMRX_EINVAL, "no tuned RF kernel for rf_taps=%d rf_decim=%d: no wide captures", c->geo.rf_taps,
                    c->geo.rf_decim);
    // the granule: the fewest narrow blocks that are a whole number of wide pairs (of staging units)
    const size_t ip = c->geo.iq_pairs;
    const size_t blocks = (size_t)up / std::gcd((size_t)up, ip), wide = blocks * ip / (size_t)up * (size_t)down;
    if (wide % 2 != 0 || wide < (size_t)rate_hist_pairs(up, down))
        return fail(FMRX_EINVAL, "capture rate %d S/s: a granule of %zu wide pairs is no whole number of staging units", cap_fs, wide);
    return set_capture_stage(c, up, down, blocks);
}

int fmrx_capture_decim(const fmrx_ctx* c, int* decim) {
    CtxLock lock_(c);
    if (!c || !decim) return fail(FMRX_EINVAL, "null argument");
    *decim = c->wide.ratio.rational() ? 0 : c->wide.ratio.down;  // D, 1 with no wide stage, 0 at a rational rate
    return FMRX_OK;
}

int fmrx_capture_rate(const fmrx_ctx* c, int* cap_fs, int* up, int* down) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (cap_fs) *cap_fs = c->wide.ratio.cap_fs(c->geo.rf_fs);
    if (up) *up = c->wide.ratio.up;
    if (down) *down = c->wide.ratio.down;
    return FMRX_OK;
}

int fmrx_wide_granule(const fmrx_ctx* c, size_t* blocks, size_t* wide_pairs) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (blocks) *blocks = c->wide.ratio.blocks;
    if (wide_pairs) *wide_pairs = wide_pairs_of(c, c->wide.ratio.blocks);
    return FMRX_OK;
}

int fmrx_tune_wide(fmrx_ctx* c, const int32_t* offsets_hz, uint64_t first_pair) {
    CtxLock lock_(c);
    if (!c || !offsets_hz) return fail(FMRX_EINVAL, "null argument");
    const CaptureRatio& r = c->wide.ratio;
    if (!r.on()) return fail(FMRX_ESTATE, "fmrx_tune_wide: the capture decimation is 1 (fmrx_set_capture_decim first)");
    if (first_pair % (uint64_t)r.down != 0) {
        if (r.rational())
            return fail(FMRX_EINVAL, "fmrx_tune_wide: first_pair %llu is no multiple of %d (the rate is %d/%d of the mode's)",
                        (unsigned long long)first_pair, r.down, r.down, r.up);
        return fail(FMRX_EINVAL, "fmrx_tune_wide: first_pair %llu is no multiple of the decimation %d",
                    (unsigned long long)first_pair, r.down);
    }
    const int rc = tune_wide(c, offsets_hz, first_pair);
    if (!rc) afc_caller_tuned(c);
    return rc;
}

int fmrx_wide_info(fmrx_ctx* c, int32_t* offsets_hz, uint64_t* next_pair, int* enabled) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (offsets_hz) std::copy(c->wide.offsets.begin(), c->wide.offsets.end(), offsets_hz);
    if (next_pair) *next_pair = c->tune.pos / (uint64_t)c->wide.ratio.up * (uint64_t)c->wide.ratio.down;
    if (enabled) *enabled = c->wide.tuned ? 1 : 0;
    return FMRX_OK;
}

}  // extern "C"
