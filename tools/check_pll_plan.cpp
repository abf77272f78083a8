// check_pll_plan.cpp — the PLL launch plan (csrc/pll_plan.cpp) checked on the CPU.
//
//   check_pll_plan grid         the plan's invariants over a grid of call shapes, trigOffsets at
//                               every form edge, knobs and demote_once (the list in check_case)
//   check_pll_plan table FILE   the plan against recorded launches: FILE is
//                               tests/golden/pll_plan_parent.json as tests/test_pll_plan.py rewrites
//                               it, a line a case:
//                                 name n_simd n_streams known trig_lo trig_hi
//                                 K (n demote_once) x K   Q (knob=value) x Q   R (kind launches steps) x R
//                               (K launch_pll calls in a row, the trigOffset advancing; R stage kinds
//                               with records).  The records per stage kind derived from the plan's
//                               steps by pll_step_stages -- the mapping launch_pll itself runs -- must
//                               equal the recorded ones.
// Prints "cases=N failures=F"; exit status 0 iff F == 0.
//
// Build: g++ -O2 -std=c++17 -ffp-contract=off tools/check_pll_plan.cpp
//            software-defined-radio-course-project_amd/csrc/pll_plan.cpp
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../software-defined-radio-course-project_amd/csrc/pll_plan.h"

using namespace fmrx;

namespace {

const PllLoop kPilot{19000.0f, 240000.0f, 2.0f, 0.0f, 0.01f};  // mode 0's stereo pilot
int g_failures = 0;

std::string describe(const PllPlanIn& in) {
    char b[256];
    std::snprintf(b, sizeof b, "n=%d ns=%d simd=%d al=%d known=%d trig=[%.0f,%.0f] spec=%d sat=%d pred=%d pipe=%d idx=%d "
                  "cnt=%d stick=%d skew=%.0f once=%d", in.n, in.n_streams, in.n_simd, in.aligned, in.known, in.trig_lo,
                  in.trig_hi, in.knobs.spec, in.knobs.sat, in.knobs.pred, in.knobs.pipe, in.knobs.idx, in.knobs.cnt,
                  in.knobs.stick, in.knobs.skew, in.demote_once);
    return b;
}

#define EXPECT(cond)                                                                            \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            if (g_failures++ < 20) std::printf("FAIL %s: %s\n  %s\n", #cond, describe(in).c_str(), where.c_str()); \
            return;                                                                             \
        }                                                                                       \
    } while (0)

// the invariants of one plan
void check_case(const PllPlanIn& in) {
    PllGeom g;
    std::vector<PllStep> steps;
    pll_plan(in, &g, &steps);
    const PllKnobs& kn = in.knobs;
    const double stick = (double)kPllTrigStick;
    // the bounds the plan goes by: the host's, shifted by the pll_hint_skew test hook
    const double hlo = std::max(in.trig_lo + kn.skew, 0.0), hhi = std::max(in.trig_hi + kn.skew, 0.0);
    const size_t n = (size_t)in.n;
    std::string where;
    size_t at = 0, dem_want = n;
    bool in_ranges = false;
    int n_demoted = 0;
    for (size_t i = 0; i < steps.size(); i++) {
        const PllStep& s = steps[i];
        char b[128];
        std::snprintf(b, sizeof b, "step %zu: op %d [%zu, +%zu) form %d cnt %d dem %d", i, (int)s.op, s.off, s.len, s.form,
                      s.cnt, s.demote_after);
        where = b;
        if (s.op == PllStep::Demoted) {  // at most one, the last, from the first range that may demote
            EXPECT(in.demote_once && i + 1 == steps.size() && ++n_demoted == 1);
            EXPECT(s.off == dem_want && s.len == n - dem_want && dem_want < n);
            continue;
        }
        // the steps tile [0, n) once, in order; segments first, in pieces of seg
        EXPECT(s.off == at && s.len > 0 && s.off + s.len <= n);
        at += s.len;
        if (s.op == PllStep::Segment) {
            EXPECT(!in_ranges && s.off % g.seg == 0 && s.len <= g.seg);
            EXPECT(s.len == g.seg || i + 1 == steps.size() || steps[i + 1].op != PllStep::Segment);
            continue;
        }
        in_ranges = true;
        // a range needs a SIMD a wave of the three-wave runner (one stream a workgroup), known and
        // equal bounds and a step inside the fast paths' domain
        EXPECT(g.spec && in.aligned && kn.spec && kn.pred && kn.pipe && g.spw == 1 && 3 * in.n_streams <= in.n_simd);
        EXPECT(in.known && hlo == hhi && std::fabs(in.step * stick) < kPllMaxPr);
        const PllForm& f = pll_form(s.form, s.cnt);
        EXPECT(f.form == s.form && f.cnt == s.cnt);  // a row of the table
        // ... the index and count runners a CU a stream, the count runner its knob's bit
        if (s.form < 20 || s.cnt) EXPECT(kPllIdxSimds * in.n_streams <= in.n_simd);
        if (s.form < 20 && !s.cnt) EXPECT(kn.idx != 0 && (kn.idx != 1 || s.form > 17));
        if (s.cnt) EXPECT(s.form <= 21 && ((kn.cnt >> (s.form - 17)) & 1));
        // every step of the range starts inside the form's domain (the trigOffset sticks at 2^24)
        EXPECT(std::min(hlo + (double)s.off, stick) >= (double)f.lo);
        EXPECT(std::min(hlo + (double)(s.off + s.len - 1), stick) <= (double)f.hi);
        // it demotes iff it is at least kPllDemoteMinIntervals of its intervals long
        const bool may_demote = s.len >= (size_t)kPllDemoteMinIntervals * (size_t)f.interval;
        EXPECT(s.demote_after == (may_demote && !in.demote_once));
        if (may_demote && in.demote_once) dem_want = std::min(dem_want, s.off);
        // a long form that stops short of its domain's end and of the call's hands a tail to the
        // 16-step form: whole intervals before it, at least kPllShortTail steps in it
        const bool to_end = s.form == kPllFormStick || s.form == kPllFormShort3 || (s.form == 22 && !kn.stick);
        const bool stops_short = s.off + s.len < n && (to_end || hlo + (double)(s.off + s.len) < (double)f.hi + 1.0);
        if (f.interval > kPllBatch && stops_short) {
            EXPECT(i + 1 < steps.size() && steps[i + 1].op == PllStep::Range);
            const PllStep& t = steps[i + 1];
            EXPECT(s.len % (size_t)f.interval == 0);
            EXPECT(!t.cnt && t.form == (s.form >= 20 ? kPllFormWide : s.form) && pll_form_interval(t.form, false) == kPllBatch);
            EXPECT(t.len >= kPllShortTail && t.len < (size_t)f.interval);
        }
    }
    where = "end";
    EXPECT(at == n);
    EXPECT(n_demoted == (dem_want < n ? 1 : 0));
}

int run_grid() {
    const int streams[] = {1, 3, 256, 257, 341, 342, 1024, 1025, 5000};
    const int lens[] = {16, 640, 1280, 4080, 4096, 4480, 16640, (1 << 18) + 640};
    std::vector<PllKnobs> knobs(1);
    auto with = [&](auto set) {
        PllKnobs k;
        set(k);
        knobs.push_back(k);
    };
    with([](PllKnobs& k) { k.spec = 0; });
    with([](PllKnobs& k) { k.sat = 0; });
    with([](PllKnobs& k) { k.pred = 0; });
    with([](PllKnobs& k) { k.pred = 2; });
    with([](PllKnobs& k) { k.pipe = 0; });
    with([](PllKnobs& k) { k.idx = 0; });
    with([](PllKnobs& k) { k.idx = 1; });
    with([](PllKnobs& k) { k.cnt = 0; });
    with([](PllKnobs& k) { k.cnt = 31; });
    with([](PllKnobs& k) { k.stick = 0; });
    with([](PllKnobs& k) { k.skew = 1048576.0; });
    with([](PllKnobs& k) { k.skew = -1048576.0; });
    struct Trig {
        bool known;
        double lo, hi;
    };
    std::vector<Trig> trigs = {{false, 0.0, 0.0}, {true, 1048576.0, 1048576.0 + 640.0}};
    for (int e : {17, 18, 19, 20, 21, 22, 24})
        for (double d : {-320.0, 0.0, 1.0}) {
            const double t = std::min(std::ldexp(1.0, e) + d, (double)kPllTrigStick);
            trigs.push_back({true, t, t});
        }
    int cases = 0;
    for (int ns : streams)
        for (int n : lens)
            for (const Trig& t : trigs)
                for (const PllKnobs& k : knobs)
                    for (int once = 0; once < 2; once++)
                        for (int aligned = 1; aligned >= 0; aligned--) {
                            check_case(PllPlanIn{n, ns, 1024, aligned != 0, pll_loop_step(kPilot), t.known, t.lo, t.hi, k,
                                                 once != 0});
                            cases++;
                        }
    // a loop whose step leaves the fast paths' domain at the stick: no range anywhere
    check_case(PllPlanIn{4480, 1, 1024, true, 30.0, true, 1048576.0, 1048576.0, PllKnobs{}, false});
    return cases + 1;
}

bool set_knob(PllKnobs& k, const std::string& name, double v) {
    if (name == "spec") k.spec = (int)v;
    else if (name == "sat") k.sat = (int)v;
    else if (name == "pred") k.pred = (int)v;
    else if (name == "pipe") k.pipe = (int)v;
    else if (name == "idx") k.idx = (int)v;
    else if (name == "cnt") k.cnt = (int)v;
    else if (name == "stick") k.stick = (int)v;
    else if (name == "skew") k.skew = v;
    else return false;
    return true;
}

int run_table(const char* path) {
    std::ifstream f(path);
    std::string line;
    int cases = 0;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        std::string name;
        PllPlanIn in{};
        int known, n_calls, n_knobs, n_kinds;
        is >> name >> in.n_simd >> in.n_streams >> known >> in.trig_lo >> in.trig_hi >> n_calls;
        std::vector<std::pair<int, int>> calls(n_calls);
        for (auto& c : calls) is >> c.first >> c.second;
        is >> n_knobs;
        bool ok = true;
        for (int q = 0; q < n_knobs; q++) {
            std::string kv;
            is >> kv;
            const size_t eq = kv.find('=');
            ok = ok && eq != std::string::npos && set_knob(in.knobs, kv.substr(0, eq), std::atof(kv.c_str() + eq + 1));
        }
        long want_launches[kStKinds] = {}, got_launches[kStKinds] = {};
        double want_steps[kStKinds] = {}, got_steps[kStKinds] = {};
        is >> n_kinds;
        for (int r = 0; r < n_kinds; r++) {
            int kind = -1;
            long la;
            double st;
            is >> kind >> la >> st;
            ok = ok && kind >= 0 && kind < kStKinds;
            if (ok) want_launches[kind] = la, want_steps[kind] = st;
        }
        ok = ok && !is.fail();
        in.known = known != 0;
        in.aligned = true;  // the engine's carrier rows: 640 floats a block
        in.step = pll_loop_step(kPilot);
        PllGeom g;
        std::vector<PllStep> steps;
        for (const auto& c : calls) {
            in.n = c.first;
            in.demote_once = c.second != 0;
            pll_plan(in, &g, &steps);
            for (const PllStep& s : steps)
                pll_step_stages(s, g, [&](int kind, double st) {
                    got_launches[kind]++;
                    got_steps[kind] += st;
                });
            // ctx.h TrigTrack::advance
            in.trig_lo = std::min(in.trig_lo + (double)in.n, (double)kPllTrigStick);
            in.trig_hi = std::min(in.trig_hi + (double)in.n, (double)kPllTrigStick);
        }
        for (int k = 0; k < kStKinds; k++)
            ok = ok && got_launches[k] == want_launches[k] && got_steps[k] == want_steps[k];
        if (!ok) {
            g_failures++;
            std::printf("FAIL %s:", name.c_str());
            for (int k = 0; k < kStKinds; k++)
                if (got_launches[k] || want_launches[k])
                    std::printf(" kind %d: %ld launches %.0f steps (recorded %ld, %.0f)", k, got_launches[k], got_steps[k],
                                want_launches[k], want_steps[k]);
            std::printf("\n");
        }
        cases++;
    }
    return cases;
}

}  // namespace

int main(int argc, char** argv) {
    int cases = 0;
    if (argc == 2 && !std::strcmp(argv[1], "grid")) cases = run_grid();
    else if (argc == 3 && !std::strcmp(argv[1], "table")) cases = run_table(argv[2]);
    else {
        std::fprintf(stderr, "usage: %s grid | table FILE\n", argv[0]);
        return 2;
    }
    std::printf("cases=%d failures=%d\n", cases, g_failures);
    return g_failures == 0 && cases > 0 ? 0 : 1;
}
