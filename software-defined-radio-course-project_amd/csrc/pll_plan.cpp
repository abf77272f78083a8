// pll_plan.cpp — the launch plan of a launch_pll call (pll_plan.h).
//
// With the host's trigOffset bounds known and equal for every stream (every context's streams
// advance together) and a SIMD for each of the three-wave runner's waves, the samples from the
// lowest self-certifying form on (2^17 with a CU a stream for the index runner, else 2^20) run as
// ranges: one self-certifying launch per form, no per-segment kernels.  The samples before, or all
// of them otherwise, run in segments: side data of the segment (parallel), the speculative runners
// by regime, pll_check_kernel, then pll_kernel resuming at the first batch that did not verify;
// the state carries in st between launches, so the steps chain exactly like one launch.
#include "pll_plan.h"

#include <algorithm>
#include <cmath>

namespace fmrx {

PllLayout pll_layout(int n, int n_streams) {
    const size_t nn = (size_t)std::max(n, 0), ns = (size_t)n_streams;
    PllLayout l;
    size_t cap = kPllSeg;
    while (cap > ((size_t)1 << 14) && cap * std::max<size_t>(ns, 1) > ((size_t)1 << 23)) cap >>= 1;
    l.seg = std::min<size_t>((nn + 15) / 16 * 16, cap);
    l.rb = l.seg / kPllBatch;
    l.args = 4 * l.seg * ns;
    l.rec = l.args + (nn * ns + 1) / 2;
    l.fail = l.rec + l.rb * ns;
    l.doubles = l.fail + (ns + 1) / 2;
    return l;
}

namespace {

// The form of a range that starts at trigOffset t, and the trigOffset at which the next form
// takes over (0: none, the form runs to the call's end): each form from the next one's lowest
// trigOffset on, the stick form (knob pll_stick) last.
int form_at(double t, bool stick, double* edge) {
    const int last = stick ? kPllFormStick : kPllFormStick - 1;
    int form = kPllFormFirst;
    while (form < last && t >= (double)pll_form(form + 1, false).lo) form++;
    *edge = form < last ? (double)pll_form(form + 1, false).lo : 0.0;
    return form;
}

}  // namespace

void pll_plan(const PllPlanIn& in, PllGeom* geom, std::vector<PllStep>* steps) {
    steps->clear();
    const PllKnobs& kn = in.knobs;
    const size_t n = (size_t)std::max(in.n, 0);
    const int n_streams = in.n_streams, n_simd = in.n_simd;
    const PllLayout lay = pll_layout(in.n, n_streams);
    PllGeom& g = *geom;
    g.seg = lay.seg;
    g.rb = lay.rb;
    g.spec = kn.spec != 0 && in.aligned;
    g.spw = 1;
    while (g.spw < 64 && (long long)g.spw * n_simd < n_streams) g.spw *= 2;
    g.waves = (n_streams + g.spw - 1) / g.spw;
    g.wpg = g.waves > n_simd / 4 ? 4 : 1;
    if (n == 0) return;
    // pll_sat = 0 / pll_pred = 0 (measurements, tests): saturated segments / segments from 2^20
    // steps on the ordinary runner too (pll_pred = 2, tests: the two-wave runner even where its
    // waves share SIMDs)
    const bool sat_ok = kn.sat != 0;
    const int pred_ok = kn.pred == 0 ? 0 : kn.pred == 2 ? 2 : 1;
    // pll_hint_skew = d (test hook): the host's trigOffset bounds shifted by d samples, so the
    // runners launched are the wrong ones.  A segment stream no runner takes keeps the pre-pass's
    // fail[] sentinel 0 and is resumed whole on the certified path; a self-certifying launch outside
    // its domain runs its range exactly (same bits either way)
    const double stick_t = (double)kPllTrigStick;
    const double hlo = std::max(in.trig_lo + kn.skew, 0.0), hhi = std::max(in.trig_hi + kn.skew, 0.0);
    const bool k = in.known && std::fabs(in.step * stick_t) < kPllMaxPr;
    // the three-wave runner: every stream at the same known trigOffset, a SIMD per wave (one
    // stream a workgroup of three); it takes the samples from trigOffset 2^20 on
    const bool pipe = g.spec && pred_ok && kn.pipe != 0 && g.spw == 1 && 3 * n_streams <= n_simd && k && hlo == hhi;
    // the index and count runners want a CU a stream; the index runner takes [2^17, 2^20)
    // (pll_idx = 0: not launched; 1: from 2^18 only, the lane runner keeping [2^17, 2^18))
    const bool cu_each = kPllIdxSimds * n_streams <= n_simd;
    const bool idx = pipe && kn.idx != 0 && cu_each;
    const double fast_min = idx ? (double)(kn.idx == 1 ? kPllIdxMin : kPllIdxMin64) : (double)kPllPipeMinLow;
    size_t n_seg = n;  // samples through the segments
    if (pipe) n_seg = hlo >= fast_min ? 0 : std::min(n, (size_t)(fast_min - hlo));

    for (size_t off = 0; off < n_seg; off += g.seg) {
        const double lo = std::min(hlo + (double)off, stick_t), hi = std::min(hhi + (double)off, stick_t);
        // the two-wave runner too wants a SIMD per wave (two of its waves on one SIMD ran slower
        // than the lane runner: 1,024 streams x 10 s 0.291 vs 0.279 s, 2,048 0.405 vs 0.371 s)
        const bool pred_fit = pred_ok && (2 * g.waves <= n_simd || pred_ok == 2);
        const bool sat_all = k && sat_ok && g.spw == 1 && lo >= stick_t;
        const bool lane = !(k && lo >= (double)kPllPredMin && (pred_fit || sat_all));
        const bool sat = sat_ok && g.spw == 1 && (!k || hi >= stick_t);
        const bool pred = pred_fit && (!k || hi >= (double)kPllPredMin) && !sat_all;
        steps->push_back({PllStep::Segment, off, std::min(g.seg, n_seg - off), lane, sat, pred, 0, false, false});
    }

    // The first interval of every form is predicted, so a long form pays nothing extra for a short
    // call: the per-block seam's 640 steps are 10 count-form intervals in [2^19, 2^20), 5 in
    // [2^20, 2^22), 5 of form 25's past 2^22.
    const bool short_call = n < kPllShortCall;
    // pll_demoted_kernel after each runner range that may demote, or with demote_once ONCE a call
    // after its runner launches, from the first such range on (a demoted stream's later launches
    // only add their steps to its hand-off): beside the pipelined engine's stage kernels each
    // launch of it waited for CUs, ~11 ms of configs[4] at one a range (profiles/r06/demote_probe/)
    size_t dem_from = n;
    auto range = [&](int form, bool cnt, size_t j, size_t e) {
        bool demote_after = false;
#ifndef FMRX_AB_NO_DEMOTED_LAUNCH  // A/B timing only (a demoted stream's range would stay unrun)
        if (e - j >= (size_t)kPllDemoteMinIntervals * (size_t)pll_form_interval(form, cnt)) {
            if (in.demote_once) dem_from = std::min(dem_from, j);
            else demote_after = true;
        }
#endif
        steps->push_back({PllStep::Range, j, e - j, false, false, false, form, cnt, demote_after});
    };
    for (size_t j = n_seg; pipe && j < n;) {
        double edge;
        int form = form_at(std::min(hlo + (double)j, stick_t), kn.stick != 0, &edge);
        size_t e = edge == 0.0 ? n : std::min((size_t)(edge - hlo), n);
        const bool cnt = form <= 21 && ((kn.cnt >> (form - kPllFormFirst)) & 1) && cu_each;
        // a short call from 2^22 on the three-candidate form in 128-step intervals: the per-block
        // seam's 640 steps are 5 of them, of 256-step ones 2 and a tail
        if (short_call && form >= 22) {
            form = kPllFormShort3;
            e = n;
        }
        // the 16-step form of the range: the index runner's own below 2^20, the wide three-wave form
        const int form16 = form >= 20 ? kPllFormWide : form;
        const size_t len = e - j, ni = (size_t)pll_form_interval(form, cnt);
        // a short call, or a range of few long intervals: on the 16-step form (from 2^20 in a short
        // call to the call's end)
        if (ni > (size_t)kPllBatch && len < kPllShortIntervals * ni) {
            if (form >= 20 && short_call) e = n;
            range(form16, false, j, e);
            j = e;
            continue;
        }
        // a long form: its whole intervals, then the tail on the 16-step form (when it is long
        // enough for one: below, it runs exactly in the long launch; on the exact path a step
        // costs ~400 ns)
        size_t body = len;
#ifndef FMRX_AB_NO_TAIL_SPLIT  // A/B: the long form's tail on its own exact path
        if (ni > (size_t)kPllBatch) {
            body = len / ni * ni;
            if (len - body < kPllShortTail) body = len;
        }
#endif
        range(form, cnt, j, j + body);
        if (body < len) range(form16, false, j + body, e);
        j = e;
    }
    if (dem_from < n) steps->push_back({PllStep::Demoted, dem_from, n - dem_from, false, false, false, 0, false, false});
}

}  // namespace fmrx
