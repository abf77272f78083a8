// fmrx_internal.h — shared declarations between the host runtime (ctx.h and the .cpp files beside it) and the HIP
// kernels (kernels.hip).  Not part of the public ABI (include/fmrx.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mono_launch.h"
#include "pll_plan.h"
#include "synth.h"

namespace fmrx {

struct ModeConstants {
    int rf_fs, rf_decim, if_fs, bp_fs, audio_up, audio_down;
};

bool mode_constants(int mode, ModeConstants* m);
void design_lpf(float* h, float fs, float fc, int taps, int gain);
void design_bpf(float* h, float fs, float fb, float fe, int taps);

constexpr int kMonoDelay = 5;   // src/project.cpp:308
constexpr int kRfFc = 100000;   // src/project.cpp:304
constexpr int kAudioFc = 16000; // src/project.cpp:305

// Halo bookkeeping: new_halo = last halo_bytes of (old_halo ++ iq), per stream.
int launch_halo_update(const uint8_t* iq, size_t stream_bytes, const uint8_t* old_halo,
                       uint8_t* new_halo, size_t halo_bytes, int n_streams, hipStream_t s);

// ---- stereo engine (REF_EXACT) kernels -----------------------------------------------
struct StereoLaunch {
    const float* demod;     // n_streams x (hist + n_if): hist demod samples precede each call
    float* channel;         // n_streams x out_stride
    float* carrier;         // n_streams x out_stride (PLL in place -> NCO)
    int n_if;               // IF samples this launch per stream
    size_t out_stride;      // floats between streams in channel / carrier (n_if, or the whole
                            //   call's when this launch is a chunk of a longer call)
    int hist;               // demod history length kept in front (>= taps-1)
    size_t demod_stride;    // floats between streams in demod
    const float* ch_c;      // bp taps, HOST memory (passed to the kernel by value)
    const float* ca_c;
    int bp_taps;
    const float* src = nullptr;  // non-null (tiled kernel only): the call's n_if new demod samples a
                                 //   stream (stride n_if, e.g. pinned host memory) are read from here
                                 //   and written into demod behind the history -- no separate copy
};
// tiled = false: the per-output kernel (A/B measurements; same bits)
int launch_bpf_pair(const StereoLaunch& L, int n_streams, hipStream_t s, bool tiled = true);
// ---- the PLL (pll.hip; its launch plan pll_plan.h, its forms pll_forms.h) ---------------------
// The scratch of a launch_pll call: `side` (pll_side_doubles(n, n_streams) doubles of device
// memory) and where its parts lie in it (pll_plan.h PllLayout, the one definition of the layout):
// one segment's side data at its start, the call's trigArgs (n floats a stream), the speculative
// runners' batch records (rb a stream) and fail[] (an int a stream).
struct PllScratch {
    double* side;
    float* args;
    float2* rec;
    int* fail;
    size_t seg, rb;
};
PllScratch pll_scratch(double* side, int n, int n_streams);
size_t pll_side_doubles(int n, int n_streams);

struct StageTimer {
    bool on = false;
    struct Rec {
        int kind;
        double steps;
        hipEvent_t a, b;
    };
    std::vector<Rec> recs;
    size_t used = 0;
    int begin(hipStream_t s) {
        if (!on) return -1;
        if (used == recs.size()) {
            Rec r{0, 0.0, nullptr, nullptr};
            if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return -1;
            recs.push_back(r);
        }
        if (hipEventRecord(recs[used].a, s) != hipSuccess) return -1;
        return (int)used++;
    }
    void end(int i, int kind, double steps, hipStream_t s) {
        if (i < 0) return;
        recs[i].kind = kind;
        recs[i].steps = steps;
        (void)hipEventRecord(recs[i].b, s);
    }
    void release() {
        for (auto& r : recs) {
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        recs.clear();
        used = 0;
    }
};

// What the host knows when it launches a PLL (ctx.h TrigTrack tracks it per context): the device's SIMD
// count (streams per wave) and, when `known`, bounds on every stream's trigOffset at the call's
// start (integer-valued, <= 2^24: the reference's float increments from a reset), so that
// launch_pll enqueues only the runners some segment can use.  Unknown (the fmrx_pll primitive's
// state lives in caller memory): every runner is launched and each takes its own waves.
struct PllHint {
    int n_simd = 1024;
    PllKnobs knobs;
    unsigned* redos = nullptr;  // fmrx_debug_pll_redos (diagnostic): n_streams x kPllRedoSlots
    bool known = false;
    double trig_lo = 0.0, trig_hi = 0.0;
    StageTimer* timer = nullptr;  // diagnostic stage timing (null: off)
    // pll_demoted_kernel once after the call's runner launches (a demoted stream's later launches
    // skip it) instead of after each runner range: the pipelined engine's chunks, where each of its
    // launches waited ~0.3 ms for CUs the stage kernels beside the chains hold
    bool demote_once = false;
};
// The PLL `loop` over n samples of n_streams streams (state st, 8 floats per stream), then the NCO
// (filter.cpp:136-174), in place.  side: device scratch of pll_side_doubles(n, n_streams) doubles.
// spec_stats (diagnostic, may be null): the speculative path adds the runner batches that did
// not verify to spec_stats[0] and the batches checked to spec_stats[1].
// nco = false: the NCO pass is left to the caller (launch_pll_nco with the same io, n, stride,
// loop, side and st, on any stream ordered after this launch and before `side` is reused).
int launch_pll(float* io, int n, int n_streams, size_t stride, const PllLoop& loop, float* st, double* side,
               hipStream_t s, const PllHint& hint, unsigned long long* spec_stats = nullptr, bool nco = true);
int launch_pll_nco(float* io, int n, int n_streams, size_t stride, const PllLoop& loop, float* st, double* side,
                   hipStream_t s);
// stereo.hip: the NCO pass alone (filter.cpp:170, parallel over samples): io[i] = cos(args[i] nco_scale +
// phase_adjust) per stream (args rows astride floats apart) and the ncoOut_state carry; the kernel
// sits beside the small audio kernel, which inlines the same arithmetic.  Enqueues only: the caller
// reads the launch status (launch_pll, launch_pll_nco).
void launch_nco_pass(float* io, int n, int n_streams, size_t stride, const float* args, size_t astride,
                     const PllLoop& loop, float* st, hipStream_t s);

// pll_sat.hip: the saturated-segment runner over a launch_pll segment (pll_spec_lane_kernel's grid
// and arguments; it runs the streams that one leaves to it)
void launch_pll_sat(dim3 grid, dim3 block, hipStream_t s, const float* io, int n, int n_streams, int spw,
                    size_t stride, const double* side, size_t seg, double step, float norm_bw, const float* st,
                    float* out, size_t ostride, int* fail, float2* rec, size_t rb, int inject);

// pll_pred.hip: the predicted-trigArg runner (segments from trigOffset 2^20, the stick included),
// pll_spec_lane_kernel's arguments, one two-wave workgroup per group of spw streams; it runs the
// groups that kernel leaves to it (pll_pred_wave)
void launch_pll_pred(int waves, hipStream_t s, const float* io, int n, int n_streams, int spw, size_t stride,
                     const double* side, size_t seg, double step, float norm_bw, const float* st, float* out,
                     size_t ostride, int* fail, float2* rec, size_t rb, int inject, int sat_ok, int pipe_on);
// The arguments of a self-certifying runner launch (pll_pipe.hip, pll_idx.hip, pll_cnt.hip) and of
// the demoted kernel that follows it (pll_demote.hip): samples [0, n) of io (stream stride `stride`)
// from the state st; their trigArgs to out (stride ostride), the exact end state to st.  inject /
// miss: the test hooks below; stats, redos (may be null): fmrx_debug_pll_stats / _redos.
struct PllRunnerArgs {
    hipStream_t s;
    const float* io;
    int n, n_streams;
    size_t stride;
    double step;
    float norm_bw;
    float* st;
    float* out;
    size_t ostride;
    int inject, miss;
    unsigned long long* stats;
    unsigned* redos;
};
// pll_pipe.hip: the three-wave runner for one stream a workgroup (spw == 1) from trigOffset 2^20,
// the stick included (pll_pipe_stream), self-certifying (no check / resume kernel): one launch runs
// the whole range and leaves the exact end state.  Its forms (pll_forms.h kPllForms: domains and
// interval lengths), by default: 22, 3 candidates, 256-step intervals (trigOffset from 2^22); 23,
// the same at the stuck trigOffset 2^24; 25, the same in 128-step intervals (short calls); 21, 5
// candidates, 128 steps ([2^21, 2^22)); 20, 5 candidates, 16 steps ([2^20, 2^21)); 24, the same
// from 2^20 to the stick.  A stream whose trigOffset is outside the form's domain runs the range on the
// exact path (a wrong host hint costs speed, not bits).  miss >= 1 / inject >= 0 (test hooks):
// a forced miss on interval `miss` / interval 1 + (inject + s) % intervals, so the exact redo
// runs.  stats (may be null): += batches redone exactly, batches run.
void launch_pll_pipe(const PllRunnerArgs& a, int form);

// pll_idx.hip: the index runner (one stream a workgroup: the chain and four evaluator waves
// for forms 17 / 18, three for form 19 -- a CU a stream, two of the five waves sharing a SIMD),
// self-certifying like launch_pll_pipe; form 17: 32 candidates ([2^17, 2^18)),
// 18: 32 ([2^18, 2^19)), 19: 16 ([2^19, 2^20)).  A stream outside the form's domain runs the
// range exactly.  Returns non-zero when the form's workgroup cannot be resident on one CU (its
// registers) or the launch fails.
int launch_pll_idx(const PllRunnerArgs& a, int form);
// pll_cnt.hip: the count runner (pll_cnt_kernel: the chain picks each step's e by one compare of
// the phase against a row of exact thresholds and a bit count), one stream a workgroup of five
// waves (a CU), self-certifying, returns as launch_pll_idx; form 17 / 18: [2^17, 2^18) /
// [2^18, 2^19), 31 candidates, 16-step intervals; 19: [2^19, 2^20), 15, 64 steps; 20: [2^20,
// 2^21), 15, 128 steps; 21: [2^21, 2^22), 7, 64 steps (pll_forms.h kPllForms, by default).
int launch_pll_cnt(const PllRunnerArgs& a, int form);
// pll_demote.hip: the rest of a self-certifying runner launch's range for the streams it demoted
// (pll_device.h pll_demote): the arguments of the runner launch it follows on stream s (miss and
// redos unused).  That launch leaves each stream's first step for this kernel in the PLL state's slot 6 (int bits; 0:
// not demoted), which this kernel clears.  One stream a workgroup: a speculative chain
// (pll_spec_lane_kernel's step) checked a sub-segment behind by the other waves, which also form
// its side data; a batch that does not verify is recomputed exactly and the chain resumes after it.
// Only a range of at least kPllDemoteMinIntervals of its form's intervals can demote: the plan
// queues pll_demoted_kernel after exactly those (PllStep::demote_after, or once a call).
int launch_pll_demoted(const PllRunnerArgs& a);
// fmrx_debug_pll_redos: per stream kPllRedoSlots u32, by the trigOffset range r of the runner's
// launch (0 [2^17, 2^20), 1 [2^20, 2^21), 2 [2^21, 2^22), 3 from 2^22, the stick included):
// slot r the intervals the self-certifying runners redid exactly, slot 4 + r the steps they ran
// demoted (pll_demote: the rest of a range on the exact path after most intervals missed).  Demoted
// steps go by the trigOffset at which the stream was demoted (state slot 5 as the runner left it):
// a later launch that only adds its steps to the hand-off (PllHint::demote_once) files them in
// that slot too, also past a range boundary; a stream's slots 4 .. 7 sum to its demoted steps
constexpr int kPllRedoSlots = 8;

// test hook: the PLL's fallback libm on device (kind 0 sincos, 1 atan2, 2 NCO cos)
int launch_pll_fallback_test(int kind, const float* a, const float* b, size_t n, float* out, hipStream_t s);

struct AudioLaunch {
    const float* demod;     // with hist samples in front (per stream stride demod_stride)
    size_t demod_stride;
    int hist;
    const float* channel;   // n_streams x n_if
    const float* nco;       // n_streams x n_if
    float* mix_tail;        // n_streams x (at-1): last mixer samples of the previous block
    float* mono_state;      // n_streams x 5
    int16_t* pcm;           // n_streams x n_blocks*2*frames
    float* mono_out;        // optional REF_EXACT mono floats
    int n_blocks, if_per_block, frames_per_block;
    int up, down, at;       // audio resampler
    const float* audio_c;
    float2* lr_out;         // optional (right, left) floats a frame, as they enter the quantiser
};
// The audio stage of blocks [b0, b1) of the call (the blocks before b0 already computed: their
// demod / channel / NCO feed b0's histories), then, when `last`, the state carry of the call's
// last block.  launch_stereo_audio: all of them.
int launch_stereo_audio_range(const AudioLaunch& L, int b0, int b1, bool last, int n_streams, hipStream_t s);
int launch_stereo_audio(const AudioLaunch& L, int n_streams, hipStream_t s);
// A few blocks a stream in ONE launch (modes 0/1, the per-block seam): the NCO from the PLL's
// trigArgs (args, astride floats a stream: pll_scratch's of a launch_pll with nco = false), the audio
// of every block in order, the state carry and the demod history move (the last demod_hist samples
// of the call to the front of its buffer); -1 when the geometry does not fit the tile.
int launch_stereo_audio_small(const AudioLaunch& L, int n_streams, const float* args, size_t astride, float nco_scale,
                              float phase_adjust, float* pll_st, int demod_hist, hipStream_t s);

// ---- RDS front half (project.cpp:200-271) ----------------------------------------------
constexpr int kRdsTaps = 51;        // bp_taps, project.cpp:307
constexpr int kRdsDelay = 5;        // rds_delay, project.cpp:309 (commented constant)
constexpr int kRdsDemodHist = 2 * (kRdsTaps - 1);  // both FIRs' history, in demod samples
constexpr int kRdsChanHist = 8;     // >= kRdsDelay channel samples kept in front
struct RdsLaunch {
    const float* demod;     // n_streams x n_if (stride demod_stride), the call's demod
    size_t demod_stride;
    float* dhist;           // n_streams x kRdsDemodHist: demod samples before this call
    float* chan;            // n_streams x (kRdsChanHist + n_if): channel, its tail in front
    size_t chan_stride;
    float* carrier;         // n_streams x n_if: BPF output, then (PLL in place) the NCO
    size_t car_stride;
    float* out;             // n_streams x n_if: mixer output
    size_t out_stride;
    float* pll;             // n_streams x 8 PLL state
    double* pll_side;       // pll_side_doubles(n_if, n_streams) scratch
    const float* ex;        // 54-60 kHz taps (device)
    const float* ca;        // 113.5-114.5 kHz taps (device)
    float bp_fs;
    int n_if;
    PllHint hint;           // the RDS PLL's (launch_pll)
};
int launch_rds(const RdsLaunch& L, int n_streams, hipStream_t s);

// ---- RDS back half (rds_bits.hip) ------------------------------------------
constexpr int kRdsbUp = 19;          // the symbol-rate resampler: 19 / (bp_fs / 2000), 38 kS/s out
constexpr int kRdsbPhaseTaps = 101;
constexpr int kRdsbTaps = kRdsbPhaseTaps * kRdsbUp;
constexpr int kRdsbWin = 2432;       // outputs a window: 152 chips of 16, 76 bits of 32
constexpr int kRdsbChips = 152;
constexpr int kRdsbSyms = 76;
constexpr int kRdsbHist = 128;       // mixer samples carried in front of a call (>= 100)
constexpr int kRdsbTail = 26;        // symbols carried: 25 bits in front of a call's first
// a stream's carried bytes: [0] last sign, [1] last chip, [2] bits seen so far (saturates at 25),
// [4 .. 4 + kRdsbTail) the last symbols, oldest first
constexpr int kRdsbStateBytes = 32;
struct RdsBitsLaunch {
    const float* mix;       // n_streams x n_if (stride mix_stride): the 57 kHz mixer output
    size_t mix_stride;
    float* hist;            // n_streams x kRdsbHist: mixer samples before this call
    uint8_t* state;         // n_streams x kRdsbStateBytes
    const float* taps;      // kRdsbTaps
    uint8_t* sign;          // scratch, n_streams x n_out
    uint8_t* winp;          // scratch, n_streams x n_win: the windows' phases
    uint8_t* lastchip;      // scratch, n_streams x n_win: the windows' last chips
    uint8_t* sym;           // scratch, n_streams x n_sym: the differential symbols
    uint8_t* bits;          // optional outputs: n_streams x n_sym, n_streams x n_sym,
    uint8_t* codes;         //   n_streams x 2 n_win (p, q), n_streams x n_out
    uint8_t* win;
    float* y;
    int down;               // bp_fs / 2000
    int n_if, n_out, n_win, n_sym;  // n_out = 2432 n_win = n_if 19 / down, n_sym = 76 n_win
};
int launch_rds_bits(const RdsBitsLaunch& L, int n_streams, hipStream_t s);

// ---- RDS block sync (rds_sync.hip) ------------------------------------------
constexpr int kRdsSyncMaxJ = 8;
constexpr int kRdsSyncCarry = 25 + 52 * kRdsSyncMaxJ;  // bits a stream carries at most, right-aligned in its row
constexpr int kRdsSyncTable = 1024;                    // burst patterns by syndrome
// A call's domain is the carried bits followed by the new ones: position d < n_carry is bit
// carry[kRdsSyncCarry - n_carry + d], the others bits[d - n_carry]; d stands for stream bit base + d.
struct RdsSyncLaunch {
    const uint8_t* bits;    // n_streams x n_new (stride bits_stride)
    size_t bits_stride;
    uint8_t* carry;         // n_streams x kRdsSyncCarry
    const uint32_t* table;  // kRdsSyncTable
    uint8_t* exact;         // scratch, n_streams x n_dom: bit u set where the position is exact for slot u
    uint32_t* cand;         // scratch, n_streams x 4 x n_dom: info16 | valid << 16 | corrected << 17 | C' << 18
    uint32_t* rec;          // scratch, n_streams x n_judge: cand | slot << 19 | votes << 21 | accepted << 31
    void* blocks;           // n_streams x max_blocks fmrx_rds_block_rec
    uint32_t* counts;       // n_streams
    unsigned long long base;  // the stream index of domain position 0
    int n_carry, n_new, n_dom;  // n_dom = n_carry + n_new
    int j0, n_judge;        // the positions judged: [j0, j0 + n_judge) of the domain
    int n_keep;             // bits carried afterwards: min(n_dom, 25 + 52 J)
    int J, V;
    unsigned max_blocks;
};
int launch_rds_sync(const RdsSyncLaunch& L, int n_streams, hipStream_t s);

// ---- FM de-emphasis (deemph.hip) -------------------------------------------
constexpr int kDeemphTaps = 64;      // the one-pole response cut where it is below half an ulp of its sum
constexpr int kDeemphHist = kDeemphTaps - 1;  // inputs carried in front of a call, per stream and channel
constexpr int kDeemphChunk = 1024;   // outputs a workgroup
// the 64 taps of fmrx_deemph_design (host only, all in double until stored); false, nothing
// written: audio_fs <= 0 or a tau_us other than 50 and 75
bool deemph_design(int audio_fs, int tau_us, float* h);
struct DeemphLaunch {
    const float* in;        // row r = (stream s, channel ch): sample i at in[s in_stride + ch + i nch]
    size_t in_stride;
    int nch;                // 1, or 2 for interleaved (right, left) frames
    size_t n;               // samples a row
    const float* h;         // kDeemphTaps taps
    const float* state_in;  // rows x kDeemphHist: the inputs in front of the call
    float* state_out;       // rows x kDeemphHist: the inputs in front of the next (never state_in)
    float* out;             // optional floats, laid out as pcm
    int16_t* pcm;           // optional S16: sample i of row r at pcm[s out_stride + ch + i nch]
    size_t out_stride;
};
int launch_deemph(const DeemphLaunch& L, int n_streams, hipStream_t s);

// ---- subcarrier meter (meter.hip) -------------------------------------------
constexpr int kMeterTones = 7;       // 17, 19, 21, 56, 58, 61, 63 kHz
constexpr int kMeterWindows = 64;    // 1 ms windows a frame
constexpr int kMeterMaxP = 288;      // samples a window: bp_fs / 1000, a multiple of 16
// P and the 7 x 2 x P table floats of fmrx_meter_design (host only, in double until stored; P and
// tables may be null); false, nothing written: bp_fs no positive multiple of 16000 or P past kMeterMaxP
bool meter_design(int bp_fs, int* P, float* tables);
struct MeterLaunch {
    const float* demod;     // n_streams rows (stride demod_stride) of frames x 64 P samples
    size_t demod_stride;
    const float* tables;    // 14 P floats: tone-major, c then s
    int P;                  // 240, 256 or 288
    int frames;             // frames a stream
    float* power;           // n_streams x frames x kMeterTones
};
int launch_meter(const MeterLaunch& L, int n_streams, hipStream_t s);

// ---- carrier sums (afc.hip) --------------------------------------------------
struct CarrierLaunch {
    const float* demod;     // n_streams rows (stride demod_stride) of frames x 64 P samples, 16-byte aligned
    size_t demod_stride;    // a multiple of 4 floats
    int P;                  // 240, 256 or 288
    int frames;             // frames a stream
    float* sums;            // n_streams x frames x 2: S, Q (8-byte aligned)
};
int launch_carrier(const CarrierLaunch& L, int n_streams, hipStream_t s);

// ---- soft stereo (blend.hip) -------------------------------------------------
constexpr int kBlendSteps = 16;      // thresholds; a level is 0 .. 16
constexpr int kBlendCarry = 8;       // floats a stream: a of the last three frames, g of them, the last level, 0
constexpr int kBlendPer = 4;         // consecutive (right, left) frames a lane of the apply kernel
// the 16 thresholds of fmrx_blend_design (host only, in double until stored); false, nothing written:
// a bound that is not finite, outside [-20, 60], or lo_db >= hi_db
bool blend_design(float lo_db, float hi_db, float* T16);
// a levels kernel's launch, soft stereo's (K = 1 level byte a frame) and quieting's (K = 2: the pair (c, m))
struct LevelsLaunch {
    const float* power;     // n_streams x frames x kMeterTones (the meter's)
    int frames;             // frames a stream, >= 1
    const float* thr;       // the stage's thresholds: kBlendSteps, or 2 x kQuietSteps (Tc, then Tm)
    const float* carry_in;  // n_streams x 8 (kBlendCarry, kQuietCarry)
    float* carry_out;       // n_streams x 8 (never carry_in)
    uint8_t* levels;        // n_streams x K (frames + 1): entry 0 the carried-in level(s), entry 1 + f frame f's
};
int launch_blend_levels(const LevelsLaunch& L, int n_streams, hipStream_t s);
struct BlendApplyLaunch {
    const float2* in;       // n_streams rows of n (right, left) frames, 16-byte aligned, n even
    unsigned n;             // frames a row; the first is frame 0 of a granule
    unsigned A, Gm;         // audio frames and meter frames a granule
    float c;                // (float)(1.0 / (32.0 A))
    const uint8_t* levels;  // n_streams rows of level_stride bytes: entry f the level in front of meter frame f
    size_t level_stride;    //   (at least the row's meter frames + 1)
    float2* out;            // optional floats (may be `in`)
    int16_t* pcm;           // optional S16 pairs, row s at pcm + 2 n s
};
int launch_blend_apply(const BlendApplyLaunch& L, int n_streams, hipStream_t s);

// ---- quieting (quiet.hip) ----------------------------------------------------
constexpr int kQuietSteps = 16;      // thresholds of the high-cut and of the soft mute; a level is 0 .. 16
constexpr int kQuietCarry = 8;       // floats a stream: n of the last three frames, the last c and m, three zeros
constexpr int kQuietTaps = 64;       // the high-cut's one-pole response, cut as de-emphasis cuts its own
constexpr int kQuietHist = kQuietTaps - 1;  // inputs carried in front of a call, per stream and channel
constexpr int kQuietChunk = 1024;    // outputs a workgroup
int launch_quiet_levels(const LevelsLaunch& L, int n_streams, hipStream_t s);
struct QuietApplyLaunch {
    const float* in;        // row (stream s, channel ch): sample i at in[s stride + ch + i nch]
    size_t stride;          // floats between the streams' rows, of `in`, `out` and `pcm` alike
    int nch;                // 1, or 2 for interleaved (right, left) frames
    unsigned n;             // frames a row; the first is frame 0 of a granule
    unsigned A, Gm;         // audio frames and meter frames a granule
    float g0, cg, cw;       // fmrx_quiet_design's gains
    const uint8_t* levels;  // n_streams rows of level_stride bytes: pair e the levels in front of meter frame e
    size_t level_stride;    //   (at least 2 (the row's meter frames + 1))
    const float* h;         // kQuietTaps taps
    const float* state_in;  // rows x kQuietHist: the inputs in front of the call
    float* state_out;       // rows x kQuietHist: the inputs in front of the next (never state_in)
    float* out;             // optional floats, laid out as `in` (never `in`)
    int16_t* pcm;           // optional S16, laid out as `in`
};
int launch_quiet_apply(const QuietApplyLaunch& L, int n_streams, hipStream_t s);

// ---- spectrum tooling and the arctan demodulator ------------------
constexpr int kPsdMaxBins = 8192;  // N complex doubles in LDS per segment
int launch_demod_arctan(float* out, double* prev, const float* i, const float* q, int n, hipStream_t s);
int launch_psd(const float* x, int nseg, int N, const float* hann, double scale, float* seg_db, float* psd,
               hipStream_t s);

// ---- generic filter.h primitives ------------------------------------------------------
int launch_resample(float* out, const float* state, const float* in, int n_in,
                    const float* coeff, int taps, int up, int down, int n_out, hipStream_t s);
// mono audio stage of every stream in one launch (project.cpp:146 + the S16 quantiser)
struct PolyStreams {
    const float* in;        // stream s: in + s in_stride, n_out outputs' inputs
    size_t in_stride;
    const float* state;     // stream s: state + s state_stride, taps - 1 floats of history
    size_t state_stride;
    const float* coeff;     // taps
    int taps, up, down, n_out;
    float* out;             // optional float output (stream s at out + s out_stride)
    size_t out_stride;
    int16_t* pcm;           // S16 output (stream s at pcm + s pcm_stride)
    size_t pcm_stride;
};
int launch_polyphase(const PolyStreams& P, int n_streams, hipStream_t s);
int launch_copy_streams(float* dst, size_t dst_stride, const float* src, size_t src_stride, int n, int n_streams,
                        hipStream_t s);
int launch_tail_copy(float* dst, const float* src, int n, hipStream_t s);
int launch_fm_demod(float* out, float* prev, const float* i, const float* q, int n,
                    hipStream_t s);
int launch_mixer(float* out, const float* a, const float* b, int n, hipStream_t s);
int launch_lr(float* l, float* r, const float* m, const float* st, int n, hipStream_t s);
int launch_normalize(const uint8_t* iq, size_t n_pairs, float* i, float* q, hipStream_t s);
int launch_quantize(const float* x, size_t n, int16_t* out, hipStream_t s);
int launch_synth(const SynthParams& p, const int16_t* d_sintab, uint64_t first, size_t n,
                 uint8_t* out, hipStream_t s);
// n_streams streams in one launch: stream k (params d_params[k]) at out + k * stride
int launch_synth_streams(const SynthParams* d_params, int n_streams, const int16_t* d_sintab,
                         uint64_t first, size_t n, uint8_t* out, size_t stride, hipStream_t s);

}  // namespace fmrx
