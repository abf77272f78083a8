// pll_forms.h — the PLL runners' regimes in one place: the trigOffset boundaries, the launch
// constants and one table row per launchable (form, runner) pair.  No HIP: the launch plan
// (pll_plan.cpp), the kernels (pll_device.h) and the stand-alone checker (tools/check_pll_plan.cpp)
// all read it.
//
// A "form" is launch_pll's number for a self-certifying runner launch: 17 .. 22 the trigOffset
// range [2^form, 2^(form + 1)) the launch is built for (22: up to the stick, 2^24, included), 23 the
// stuck trigOffset itself, 24 the wide 16-step three-wave form (any trigOffset from 2^20), 25 the
// three-candidate form in short intervals (a short call from 2^22).  The index runner
// (launch_pll_idx) takes forms 17 .. 19, the three-wave runner (launch_pll_pipe) 20 .. 25, the count
// runner (launch_pll_cnt) 17 .. 21 where knob pll_cnt's bit form - 17 is set.
#pragma once
#include <stddef.h>

namespace fmrx {

// filter.cpp:165-166: the float trigOffset sticks at 2^24 (trigOffset + 1.0f == trigOffset from here,
// 69.9 s into a stream at 240 kS/s)
constexpr float kPllTrigStick = 16777216.0f;
// the fast paths' bound on |pr_j| = |step x trigOffset| (pll_math.h pll_side); a loop whose step
// reaches it at the stick runs on the exact path alone
constexpr double kPllMaxPr = 4.0e8;

// NB samples per optimistic batch.  Measured (10 s mode-0 stereo): NB = 16 beats 8 and 12.  The
// certification is ~23 % of the step: without it the loop runs 0.31 s instead of 0.40 s.
constexpr int kPllBatch = 16;
// at most this many samples per stream per PLL segment (pll_layout)
constexpr size_t kPllSeg = (size_t)1 << 18;

// ---- regime boundaries (trigOffset at a segment's or a range's first step) ----------------------
// the two-wave predicted runner (pll_pred_kernel): segments from here, the stick included
constexpr float kPllPredMin = 1048576.0f;  // 2^20
// the three-wave runner (pll_pipe_kernel): three candidates from kPllPipeMin, five in long
// intervals in [kPllPipeMin5, kPllPipeMin), five in 16-step intervals in [kPllPipeMinLow, kPllPipeMin5)
constexpr float kPllPipeMin = 4194304.0f;     // 2^22
constexpr float kPllPipeMin5 = 2097152.0f;    // 2^21
constexpr float kPllPipeMinLow = 1048576.0f;  // 2^20
// the index runner's lowest trigOffset: 2^17 (kPllIdxMin64; 2^18, kPllIdxMin, with FMRX_PLL_IDX=1).  In
// [2^17, 2^18) 32 candidates (c0 - 16 .. c0 + 15) run 62 ns a step with their misses redone,
// against the lane runner's 75; 64 took 113 (1,024 candidate evaluations an interval on three
// evaluator waves, profiles/r04/val/stages.json; profiles/r04/ab_idx17_nc32/)
constexpr float kPllIdxMin = 262144.0f;    // 2^18
constexpr float kPllIdxMin64 = 131072.0f;  // 2^17
constexpr float kPllIdx19Min = 524288.0f;  // 2^19: the 16-candidate index form, the 15-candidate count form

// ---- launch rules (pll_plan) --------------------------------------------------------------------
constexpr int kPllIdxSimds = 4;  // SIMDs a stream of the index / count runner takes: one CU
// only a runner launch of at least this many intervals demotes (the plan queues the demoted kernel
// after exactly those: a shorter range cannot pay for it, e.g. the per-block seam's 640 steps)
constexpr int kPllDemoteMinIntervals = 64;
// a range of fewer than kPllShortIntervals of its form's long intervals runs on the 16-step forms
// (in a call of fewer than kPllShortCall steps a stream, to the call's end); a long form's tail
// past its last whole interval of at least kPllShortTail steps runs on the 16-step form (three
// 16-step intervals; a long launch needs two whole intervals or it runs exactly)
constexpr size_t kPllShortCall = 4096, kPllShortIntervals = 2, kPllShortTail = 48;

// ---- interval lengths (tunable per build: make ab AB=-DFMRX_...) --------------------------------
#ifndef FMRX_STICK_BPI
#define FMRX_STICK_BPI 16  // batches an interval of the stick form: 256-step intervals (8: 128, 4: 64)
#endif
#ifndef FMRX_PIPE22_BPI
#define FMRX_PIPE22_BPI 16  // batches an interval of the three-candidate form below the stick (256 steps)
#endif
#ifndef FMRX_PIPE21_BPI
#define FMRX_PIPE21_BPI 8  // batches an interval of the five-candidate [2^21, 2^22) form (128 steps)
#endif
#ifndef FMRX_PIPE25_BPI
#define FMRX_PIPE25_BPI 8  // batches an interval of the short-call three-candidate form (128 steps: 640 = 5)
#endif
#ifndef FMRX_CNT17_NI
#define FMRX_CNT17_NI 16  // steps an interval of the [2^17, 2^19) count forms (off by default)
#endif
#ifndef FMRX_CNT19_NI
#define FMRX_CNT19_NI 64  // steps an interval of the [2^19, 2^20) count form
#endif
#ifndef FMRX_CNT20_NI
#define FMRX_CNT20_NI 128  // steps an interval of the [2^20, 2^21) count form (two rows of counts)
#endif
#ifndef FMRX_CNT21_NI
#define FMRX_CNT21_NI 64  // steps an interval of the [2^21, 2^22) count form
#endif

// Per-stage device time of the stereo engine (fmrx_debug_stage_timing; diagnostic): HIP event
// pairs recorded on the stream each stage is launched on, read after the call.  Runner records
// carry the serial steps they ran when they were the only runner of their segment (the host's
// trigOffset bounds put every stream in that runner's regime), so ns per step per regime is
// measured, not modelled.
enum StageKind {
    kStFront, kStBpf, kStPrep, kStLane, kStPred, kStSat, kStPipe20, kStPipe21, kStPipe22, kStCheck, kStTail,
    kStNco, kStAudio, kStIdx17, kStIdx18, kStIdx19, kStCnt17, kStCnt18, kStCnt19, kStCnt20, kStCnt21, kStStick, kStKinds
};

// One launchable (form, runner) pair: the trigOffsets [lo, hi] of a range's first step the launch
// is built for (a stream outside them runs the range on the exact path: a wrong host hint costs
// speed, not bits), the steps of one of its intervals and the stage kind its time is filed under.
struct PllForm {
    int form;
    bool cnt;  // the count runner's launch of the form
    float lo, hi;
    int interval;
    StageKind kind;
};
constexpr PllForm kPllForms[] = {
    // the index runner: 16-step intervals, 32 / 32 / 16 candidates
    {17, false, kPllIdxMin64, kPllIdxMin - 1.0f, kPllBatch, kStIdx17},
    {18, false, kPllIdxMin, kPllIdx19Min - 1.0f, kPllBatch, kStIdx18},
    {19, false, kPllIdx19Min, kPllPipeMinLow - 1.0f, kPllBatch, kStIdx19},
    // the three-wave runner: five candidates (20, 21, 24), three (22, 23, 25)
    {20, false, kPllPipeMinLow, kPllPipeMin5 - 1.0f, kPllBatch, kStPipe20},
    {21, false, kPllPipeMin5, kPllPipeMin - 1.0f, kPllBatch * FMRX_PIPE21_BPI, kStPipe21},
    {22, false, kPllPipeMin, kPllTrigStick, kPllBatch * FMRX_PIPE22_BPI, kStPipe22},
    {23, false, kPllTrigStick, kPllTrigStick, kPllBatch * FMRX_STICK_BPI, kStStick},
    {24, false, kPllPipeMinLow, kPllTrigStick, kPllBatch, kStPipe20},
    {25, false, kPllPipeMin, kPllTrigStick, kPllBatch * FMRX_PIPE25_BPI, kStPipe22},
    // the count runner: 31 / 31 / 15 / 15 / 7 candidates
    {17, true, kPllIdxMin64, kPllIdxMin - 1.0f, FMRX_CNT17_NI, kStCnt17},
    {18, true, kPllIdxMin, kPllIdx19Min - 1.0f, FMRX_CNT17_NI, kStCnt18},
    {19, true, kPllIdx19Min, kPllPipeMinLow - 1.0f, FMRX_CNT19_NI, kStCnt19},
    {20, true, kPllPipeMinLow, kPllPipeMin5 - 1.0f, FMRX_CNT20_NI, kStCnt20},
    {21, true, kPllPipeMin5, kPllPipeMin - 1.0f, FMRX_CNT21_NI, kStCnt21},
};
constexpr int kPllFormFirst = 17, kPllFormStick = 23, kPllFormWide = 24, kPllFormShort3 = 25;

// the row of a launchable pair (the callers pass the plan's forms only; any other pair: the first row)
constexpr const PllForm& pll_form(int form, bool cnt) {
    for (const PllForm& f : kPllForms)
        if (f.form == form && f.cnt == cnt) return f;
    return kPllForms[0];
}
// steps an interval of a form on the count runner (cnt) or the index / three-wave runner
constexpr int pll_form_interval(int form, bool cnt) { return pll_form(form, cnt).interval; }

}  // namespace fmrx
