// pll_plan.h — what a launch_pll call launches, decided apart from launching it.  No HIP: pure
// integer and double arithmetic on the call's shape, the host's trigOffset bounds and the knobs,
// so the decision is checked on the CPU (tools/check_pll_plan.cpp, tests/test_pll_plan.py).
// launch_pll (pll.hip) builds the plan and maps each step to its kernels.
#pragma once
#include <stddef.h>

#include <vector>

#include "pll_forms.h"

namespace fmrx {

// The count runner's forms by default: [2^19, 2^20) and [2^20, 2^21) (bits 2, 3).  Same-box A/B,
// two alternating rounds (profiles/r05/ab_cnt12/): one 10 s stream 0.1093 -> 0.0923 s, configs[4]
// 0.430 -> 0.418 s, configs[2] 1.240 -> 1.222 s.  [2^17, 2^19) stay on the index runner (the
// count form's 31-candidate evaluators bound it: 68-73 ns a step against 55), [2^21, 2^22) on the
// three-wave runner (profiles/r05/rprof/).
constexpr int kPllCntDefault = 12;

// Per-context switches of the PLL launch (ctx.h fmrx_ctx::knobs; fmrx_debug_set_knob).  The
// tuning ones pick which runners run (same bits either way) and are read from the environment
// once, when the context is created; the test hooks make the runners do extra (redone) work --
// the output stays the exact path's -- and are set only through fmrx_debug_set_knob.
struct PllKnobs {
    int spec = 1;        // 0: the plain certified launch (FMRX_PLL_SPEC)
    int sat = 1;         // 0: no saturated-segment runner (FMRX_PLL_SAT)
    int pred = 1;        // 0: no predicted runners; 2: the two-wave one even where waves share SIMDs
    int pipe = 1;        // 0: no three-wave runner (FMRX_PLL_PIPE)
    int idx = 2;         // index runner from 2^17 (2), from 2^18 (1), off (0) (FMRX_PLL_IDX)
    int cnt = kPllCntDefault;  // bit f - 17: the count runner takes form f's range (FMRX_PLL_CNT)
    int stick = 1;       // the three-candidate runner's stick form past trigOffset 2^24 (FMRX_PLL_STICK)
    int inject = -1;     // test hook: the runners corrupt batch 1 + (k + s) % (nb - 1) of stream s
    int pipe_miss = -1;  // test hook: the self-certifying runners report interval k as missed
    double skew = 0.0;   // test hook: the host's trigOffset bounds shifted by this many samples
};

// The loop a launch_pll call runs (filter.cpp:136's arguments): the stereo pilot's
// {19000, if_fs, 2, 0, 0.01} (project.cpp:166), the RDS carrier's {114000, bp_fs, 0.5, 0, 0.01}.
struct PllLoop {
    float freq, fs, nco_scale, phase_adjust, norm_bw;
};
// filter.cpp:163: 2*PI*(freq/Fs) in double from the float quotient (host == device IEEE)
inline double pll_loop_step(const PllLoop& l) {
    return (2.0 * 3.14159265358979323846) * static_cast<double>(l.freq / l.fs);  // dy4.h:14 PI
}

// The scratch of a launch_pll call (`side`), in doubles from its start: one segment's side data
// (iv, pr, half turns: 3 seg, plus seg as slack for the stream-minor layout) first, then at `args`
// the call's trigArgs (n floats a stream: every runner writes its steps' trigArgs there, the NCO
// reads them once at the end), at `rec` the speculative runners' batch records (rb = seg / 16
// float2 a stream), at `fail` their first unverified batch (an int a stream); `doubles` in all.
// Segment length `seg` (the lane / two-wave / saturated runners, checked by pll_check_kernel):
// kPllSeg samples up to 32 streams, then shorter so that segment x streams stays ~2^23 (down to
// 2^14): a batch the runner got wrong (~3e-9 of steps) costs the rest of its segment on the
// certified path, serially, so the expected cost per segment grows with segment^2 x streams.  The
// self-certifying runners need no segments.
struct PllLayout {
    size_t seg, rb, args, rec, fail, doubles;
};
PllLayout pll_layout(int n, int n_streams);

struct PllPlanIn {
    int n, n_streams, n_simd;
    bool aligned;  // io 16-byte aligned and stride % 4 == 0 (the speculative runners' vector loads)
    double step;   // pll_loop_step
    bool known;    // the host's trigOffset bounds (PllHint)
    double trig_lo, trig_hi;
    PllKnobs knobs;
    bool demote_once;
};
// The launch geometry every step of a call shares: streams per wave (one while the waves fit one per
// SIMD, then a power of two), waves, waves per workgroup (past 256 waves, workgroups of 4 waves,
// one per SIMD of a CU: 64-lane workgroups alone were placed two to a SIMD at 1,024 waves, half
// speed for both), and whether the speculative runners run at all (knob pll_spec, aligned rows).
struct PllGeom {
    size_t seg, rb;
    int spw, waves, wpg;
    bool spec;
};
// One step of the plan, samples [off, off + len) of every stream; the steps tile [0, n) in order,
// but for a last Demoted step, which covers the ranges from its `off` again.
struct PllStep {
    enum Op { Segment, Range, Demoted } op;
    size_t off, len;
    // Segment: side data, the speculative runners it can need, the check and the certified resume.
    // With known trigOffset bounds only the runners some stream of the segment can take are set:
    // the lane runner, the saturated one (pll_sat_segment), the two-wave one (pll_pred_wave)
    bool lane, sat, pred;
    // Range: one self-certifying launch of `form` (pll_forms.h) on the count runner (cnt) or the
    // index / three-wave runner; demote_after: pll_demoted_kernel over the same range follows it
    int form;
    bool cnt, demote_after;
    // Demoted: pll_demoted_kernel once, after the call's last runner launch (PllPlanIn::demote_once)
};

// The plan of a call: `geom` and the steps, appended to `steps` after clearing it (no allocation
// once its capacity has grown to a call's steps: a segment every `seg` samples, a few ranges).
void pll_plan(const PllPlanIn& in, PllGeom* geom, std::vector<PllStep>* steps);

// The stage records (fmrx_debug_stage_timing) of a step, f(kind, steps) in launch order: exactly
// one per launch group of launch_pll, which launches what this function names.  A segment
// runner's steps count toward its regime only when it is the segment's one runner.
template <class F>
inline void pll_step_stages(const PllStep& st, const PllGeom& g, F&& f) {
    if (st.op == PllStep::Demoted) return f(kStTail, 0.0);
    if (st.op == PllStep::Range) return f(pll_form(st.form, st.cnt).kind, (double)st.len);
    f(kStPrep, 0.0);
    if (g.spec) {
        if (g.spw <= 4) {  // the split kernels
            const double one = (int)st.lane + st.sat + st.pred == 1 ? (double)st.len : 0.0;
            if (st.lane) f(kStLane, one);
            if (st.sat) f(kStSat, one);
            if (st.pred) f(kStPred, one);
        } else {
            f(kStLane, (double)st.len);  // pll_spec_kernel
        }
        if (st.len >= (size_t)kPllBatch) f(kStCheck, 0.0);
    }
    f(kStTail, 0.0);
}

}  // namespace fmrx
