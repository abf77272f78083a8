// pll_runner.h — what the predicted-trigArg PLL runners share (pll_pred.hip, pll_pipe.hip,
// pll_idx.hip, pll_cnt.hip: one translation unit a runner, each with its own copy of this header's
// anonymous namespace).  Device code: a candidate's e and its certification, the phase thresholds,
// the exact path's e after an exact stretch, the frame of the index and count runners.  Host code:
// the one launch template of the index and count forms.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "dsp_device.h"
#include "fmrx_internal.h"
#include "pll_device.h"
#include "pll_math.h"

// A/B build only (Makefile `ab`, AB=-DFMRX_AB_PROF): shader-clock cycles of a runner's waves, body
// vs barrier wait, summed over every batch and workgroup; each runner's file keeps its own counters
// and prints them at exit.  PROF_ADD(on, counter, v): the lanes with `on` add v to the counter (in
// the product build the counters do not exist and v is only named)
#ifdef FMRX_AB_PROF
#define PROF_T() __builtin_amdgcn_s_memtime()
#define PROF_ADD(on, counter, v) do { if (on) atomicAdd(&(counter), v); } while (0)
#else
#define PROF_T() 0ull
#define PROF_ADD(on, counter, v) ((void)(v))
#endif

namespace fmrx {
namespace {

// e of a step (input v, 1/v = iv, half turn h = 0.5 [v < 0]) whose previous trigArg is a:
// pll_spec_lane_kernel's step with both sin and cos in this lane.
__device__ inline float pred_e(float a, float v, double iv) {
    const double x = (double)a;
    const double nd = rint(x * kInvPio2);
    const double r = fma(-nd, kPio2Lo, fma(-nd, kPio2Hi, x));
    const double z = r * r;
    const double sn = r * split_w_horner(z, split_coef(false));
    const double cs = split_w_horner(z, split_coef(true));
    const float fc = (float)cs, nfs = -(float)sn;
    const float2v ab = float2v{fc, nfs} * v;
    const double Y = fma((double)ab.x, sn, (double)ab.y * cs);
    const double h = iv < 0.0 ? 0.5 : 0.0;
    const double B = pll_offset_h(x, h);
    return (float)fma(Y, iv, B);
}

// Adjacent floats, across zero too (the phase may sit near it).
__device__ inline float f_up(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u == 0x80000000u ? 1u : u - 1u) : u + 1u);
}
__device__ inline float f_down(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return __builtin_bit_cast(float, (u & 0x80000000u) ? u + 1u : (u == 0u ? 0x80000001u : u - 1u));
}

// trigArg = float(P + phase) in double (filter.cpp:165) is monotone in the float phase, so
// "trigArg >= c" is "phase >= T" for a float threshold T: the smallest phase whose trigArg
// reaches c.  The chain then selects its candidate with float compares of the phase it has just
// formed, before the double sum and its roundings.  T lies within an ulp of float(m - P), m the
// boundary of c's rounding interval (the midpoint with its predecessor, the tie rounding to
// even): the first of its two lower neighbours, itself and its upper neighbour that reaches c,
// checked by the double sum itself, exactly; -inf flags a T outside that window (the caller
// poisons the step's candidates, so the chain takes it as a miss).
__device__ inline bool reaches(double P, float ph, float c) { return (float)(P + (double)ph) >= c; }
__device__ inline float phase_thr(double P, uint32_t cb) {
    const float c = __builtin_bit_cast(float, cb);
    const double m = 0.5 * ((double)__builtin_bit_cast(float, cb - 1u) + (double)c);
    const float f0 = (float)(m - P), fm = f_down(f0), fmm = f_down(fm), fp = f_up(f0);
    const bool rp = reaches(P, fp, c), r0 = reaches(P, f0, c), rm = reaches(P, fm, c), rmm = reaches(P, fmm, c);
    const float T = rm ? fm : (r0 ? f0 : fp);
    return (rp && !rmm) ? T : -__builtin_inff();
}

// The chain's candidate choice, e of trigArg_{j-1} from the phase: a = (T0, T1, e(c0 - 1),
// e(c0)), ep = e(c0 + 1); phase >= T1 -> c0 + 1, >= T0 -> c0, else c0 - 1.  One asm block: two
// compares into SGPR masks, then the two v_cndmask, with the two wait states a VALU-written lane
// mask needs before a VALU reads it (the s_nop and the first v_cndmask stand between each compare
// and its reader).  Left to itself the compiler writes VCC twice, each with its own wait states;
// as separate statements it pads each one (tools/ubench_chain.hip, modes 6 and 9).
__device__ inline float pick(float phase, float4 a, float ep) {
    float e;
    uint64_t m0, m1;
    asm("v_cmp_ge_f32_e64 %1, %3, %4\n"
        "v_cmp_ge_f32_e64 %2, %3, %5\n"
        "s_nop 0\n"
        "v_cndmask_b32_e64 %0, %6, %7, %1\n"
        "v_cndmask_b32_e64 %0, %0, %8, %2"
        : "=&v"(e), "=&s"(m0), "=&s"(m1)
        : "v"(phase), "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(ep));
    return e;
}

// pred_e with pll_batch_fast's certification of one step: the float roundings of the
// candidate's cos and sin (16-ulp margin), |r| >= kPllMinR, |a| < kPllMaxX, [th - E, th + E]
// within one float (E = kPllEBatch: d = Y iv with the rcp-Newton 1/v), |d| < kPllMaxD, |B| <=
// kPllMaxB, a finite iv.  ok: e is then the exact path's e (pll_step, glibc's atan2 rounded) for
// a step with input v after trigArg a, bit for bit.
__device__ inline float pred_e_cert(float a, float v, double iv, bool& ok) {
    const double x = (double)a;
    const double nd = rint(x * kInvPio2);
    const double r = fma(-nd, kPio2Lo, fma(-nd, kPio2Hi, x));
    const double z = r * r;
    const double sn = r * split_w_horner(z, split_coef(false));
    const double cs = split_w_horner(z, split_coef(true));
    const float fc = (float)cs, nfs = -(float)sn;
    const float2v ab = float2v{fc, nfs} * v;
    const double Y = fma((double)ab.x, sn, (double)ab.y * cs);
    const double h = iv < 0.0 ? 0.5 : 0.0;
    const double B = pll_offset_h(x, h);
    const double d = Y * iv;
    const double th = d + B;
    const float lo = (float)(th - kPllEBatch), hi = (float)(th + kPllEBatch);
    ok = (int)(fabs(x) < kPllMaxX) & (int)(pll_margin16x8(cs) > 256u) & (int)(pll_margin16x8(sn) > 256u) &
         (int)(fabs(r) >= kPllMinR) & (int)(lo == hi) & (int)(fabs(d) < kPllMaxD) & (int)(fabs(B) <= kPllMaxB);
    return lo;
}

// 1 / v as the check kernel forms it (reciprocal + one Newton step, ~2^-46 relative, within the
// batch bound kPllEBatch); NaN outside [kPllMinV, 1e300) (pll_side)
__device__ inline double pll_iv(float v) {
    const double vd = (double)v;
    const double r0 = __builtin_amdgcn_rcp(vd);
    const double r1 = fma(r0, fma(-vd, r0, 1.0), r0);
    return (fabs(vd) >= (double)kPllMinV && fabs(vd) < 1.0e300) ? r1 : (double)NAN;
}

// The exact path's e of a step with input v whose previous trigArg is a (pll_step's first half
// from the state after that trigArg: its sin/cos certified or from the library, then the
// rotation atan2 certified or from the library).  Used where the chain continues after an exact
// stretch, by the chain and by wave 2's replay alike.
__device__ __noinline__ float exact_e(float a, float v) {
    const DeviceLib lib;
    PllCtx c{};
    float sv, cv;
    if (!sincos_ctx_f(a, &sv, &cv, &c)) lib.sincosf_(a, &sv, &cv);
    const float eI = v * cv;
    const float eQ = v * (-sv);
    float e;
    if (!rot_atan2_f(eQ, eI, c, &e)) e = lib.atan2f_(eQ, eI);
    return e;
}

// The e of a range's first step from the state it starts with (pll_step's first half with the
// state's own feedback, no sincos context: the library atan2, as pll_redo's first step).
__device__ __noinline__ float exact_e_fb(float fbI, float fbQ, float v) {
    const DeviceLib lib;
    const float eI = v * fbI;
    const float eQ = v * (-fbQ);
    return lib.atan2f_(eQ, eI);
}

// Never launched.  The out-of-line exact path (pll_redo, pll_device.h) is compiled once a file, for
// the callers it has there: LLVM folds an argument they all pass alike into it (the self-certifying
// runners always write; the two-wave runner always starts from an empty context) and bounds it by
// the union of their launch bounds.  Its code, and through the registers it clobbers that of every
// kernel calling it, would depend on which runners share a file.  This caller gives every file what
// the four runners together give: a write flag and a context known only at run time, work groups up
// to 320 threads.  Each runner's exact path is then, to the instruction, what it was in one file.
__global__ void __launch_bounds__(320) pll_exact_path_callers(const float* x, float* out, int n, float* st, double step) {
    PllPair r{PllState{st[0], st[1], st[2], st[3], st[5]}, PllCtx{}};
    for (int k = 0; k < 2; k++) r = pll_redo(r.p, r.ctx, x, out, n, st[6], st[7], step, st[4] != 0.0f);
    st[0] = r.p.integ;
    st[1] = r.p.phase;
}

// A/B build only (make ab AB=-DFMRX_AB_NODEMOTE): the index and count runners without pll_demote's
// checks (timing of the locked path; an unlocked stream then redoes every interval)
#ifdef FMRX_AB_NODEMOTE
constexpr bool kAbNoDemote = true;
#else
constexpr bool kAbNoDemote = false;
#endif

// ---- the frame of the index and count runners (pll_idx_kernel, pll_cnt_kernel) -------------------
//
// One stream a workgroup, wave 0 the chain and the others its evaluators.  What the two kernels do
// alike around their chain and evaluator loops, once; what differs between them is a parameter.
// (pll_pipe_kernel keeps its own copy: folded, one of its stages missed the timing bar.)

// The stream of this workgroup and its range: input and trigArg rows from the range's first sample,
// the state (S: read at the start, the exact end state written), the loop gains, the state and
// trigOffset the range starts with, the range's steps.
struct PllStream {
    const float* x;
    float* out;
    float* S;
    float Ki, Kp;
    PllState p;
    float trig0;
    double step;
    int n, s;
    // pll_side's P of step j (trigOffset after the step's increment, stuck at 2^24)
    __device__ __forceinline__ double pr_at(long long j) const {
        return step * (double)(float)fmin((double)trig0 + (double)(j + 1), (double)kPllTrigStick);
    }
    // steps [j0, j1) exactly from state q (c): outputs
    __device__ __forceinline__ void exact(PllState& q, PllCtx& c, long long j0, long long j1) const {
        if (j1 > j0) {
            const PllPair z = pll_redo(q, c, x + j0, out + j0, (int)(j1 - j0), Ki, Kp, step, true);
            q = z.p;
            c = z.ctx;
        }
    }
};

// test hook (knob pll_inject = k): a forced miss on interval 1 + (k + s) % ni of stream s (the exact
// redo runs; counted as resumed), -1 off
__device__ __forceinline__ int pll_hook_inject(int inject, int s, int ni) {
    return inject >= 0 && ni > 0 ? 1 + (inject + s) % ni : -1;
}

// The kernel's arguments as the stream f of workgroup blockIdx.x (grid = n_streams).  The state is
// uniform over the group (readfirstlane): the form's domain test and every branch and loop after it
// stay scalar.  True (return now): the stream was demoted by an earlier runner launch of this call
// (pll_demote; state slot 6: the steps it left to pll_demoted_kernel, int bits) -- this range is
// theirs too, add it and leave (uniform).
__device__ __forceinline__ bool pll_stream_open(PllStream& f, const float* io, int n, size_t stride, double step,
                                                float norm_bw, float* st, float* out_base, size_t ostride,
                                                unsigned* redos) {
    const int s = blockIdx.x;
    float* S = st + 8 * (size_t)s;
    const float Kp = norm_bw * static_cast<float>(2.666);
    const float Ki = (norm_bw * norm_bw) * static_cast<float>(3.555);
    auto uni = [](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); };
    const PllState p{uni(S[0]), uni(S[1]), uni(S[2]), uni(S[3]), uni(S[5])};
    f = PllStream{io + (size_t)s * stride, out_base + (size_t)s * ostride, S, Ki, Kp, p, p.trig, step, n, s};
    if (const int rem = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, S[6])); rem > 0) {
        if (threadIdx.x == 0) {
            S[6] = __builtin_bit_cast(float, rem + n);
            if (redos) atomicAdd(&redos[kPllRedoSlots * (size_t)s + 4 + pll_redo_range(p.trig)], (unsigned)n);
        }
        return true;
    }
    return false;
}

// A short range (fewer than two intervals), or a stream outside the form's domain (the host's
// trigOffset bounds were wrong: costs speed, never bits): every step exactly on wave w = 0 (no
// barrier is reached); the kernel returns after it.  `run` batches counted, outside the domain as
// "resumed" on the exact path too.
__device__ __forceinline__ void pll_stream_all_exact(PllStream& f, int w, int t, bool in_domain, unsigned long long run,
                                                     unsigned long long* stats) {
    if (w == 0) {
        PllCtx c{};
        c.valid = false;
        f.exact(f.p, c, 0, f.n);
        if (t == 0) {
            float* S = f.S;
            S[0] = f.p.integ; S[1] = f.p.phase; S[2] = f.p.fbI; S[3] = f.p.fbQ; S[5] = f.p.trig;
            S[6] = 0.0f;  // not demoted (pll_demoted_kernel)
            if (stats) {
                if (!in_domain) atomicAdd(stats, run);
                atomicAdd(stats + 1, run);
            }
        }
    }
}

// The chain's start (interval 1 starts at the range's first step, predicted from the start phase
// like every other; until round 6 a whole interval ran first on the exact path, at ~400 ns a step):
// step 0's e from the state's feedback (every lane), returned; the start state in ring slot 0 --
// its verdict (z) reads as a hit (no prediction pll_demote counts), and no i >= 2 test in the
// evaluators' loop (LLVM peels a whole unrolled iteration for one); the prologue's barrier.
__device__ __forceinline__ float pll_chain_begin(const PllStream& f, int t, float4 (&sst)[4], int (&sexact)[4]) {
    const float e = exact_e_fb(f.p.fbI, f.p.fbQ, f.x[0]);
    if (t == 0) {
        sst[0] = make_float4(f.p.integ, f.p.phase, 0.0f, 0.0f);
        sexact[0] = 1;
    }
    __syncthreads();  // (prologue)
    return e;
}

// pll_demote for a chain that has each interval's verdict at its end: hist, the verdicts of its last
// 32 intervals (SGPR bits), takes interval i - 1's (prev_bad); past MISSES of them the chain leaves
// after interval i (true) and the demoted kernel runs the rest.  The verdicts up to interval i - 1
// decide it: scalar work at the interval's start, off the chain's path (at its end it delayed the
// barrier).  Only at the end of an evaluators' group of RD intervals, with an interval still ahead,
// in a range of kPllDemoteMinIntervals intervals of STEPS steps, and only from a state the demoted
// kernel's fast batches take: beyond their range every interval misses for that reason alone, and
// the exact path is what runs either way; the range test only then, the common path SALU work only.
// (RD, STEPS and MISSES as template arguments: as run-time ones of this function LLVM turned the
// short-circuit test into selects before inlining it, five more instructions an interval.)
template <int RD, int STEPS, int MISSES>
__device__ __forceinline__ bool pll_chain_leaves(uint32_t& hist, uint32_t prev_bad, int i, int ni, int n, float integ,
                                                 float phase) {
    hist = (hist << 1) | prev_bad;
    bool leave = false;
    if (!kAbNoDemote && i % RD == 0 && i < ni && n >= kPllDemoteMinIntervals * STEPS &&
        __builtin_popcount(hist) >= MISSES)  // (scalar, nearly always false: a branch
        leave = __builtin_amdgcn_ballot_w64(fabsf(phase) < kPllMaxPhase && fabsf(integ) < kPllMaxInteg) != 0;
    return leave;
}

// The exact redo of interval i (`steps` steps an interval) from the state at its start, (integ0,
// phase0) -- interval 1: the range's start state as given; the chain stores it.  Leaves the
// interval's exact end in (integ, phase) and returns its last trigArg.
__device__ __forceinline__ float pll_redo_interval(const PllStream& f, int i, int steps, float integ0, float phase0,
                                                   float& integ, float& phase) {
    const int j0 = steps * (i - 1);
    PllState q = f.p;
    PllCtx c{};
    c.valid = false;
    if (i > 1) {
        const float a = (float)(f.pr_at(j0 - 1) + (double)phase0);  // the trigArg before it
        pll_state_at(q, c, integ0, phase0, f.trig0, (long long)j0, a, DeviceLib{});
    }
    f.exact(q, c, j0, j0 + steps);
    integ = q.integ;
    phase = q.phase;
    return (float)c.x;
}

// The end of the chain of the index and count runners after its last interval (`last`: ni, or the
// interval it left after when demoted): the steps past it exactly, from the end state -- or,
// demoted, the exact state at jf and its step for pll_demoted_kernel (pll_demote.hip), which runs
// the rest.  Then, lane 0: the exact end state, the steps left to pll_demoted_kernel in slot 6 (int
// bits; 0: not demoted), fmrx_debug_pll_stats (batches `resumed`, batches `run`) and
// fmrx_debug_pll_redos (slot: the trigOffset range the launch files under).
__device__ __forceinline__ void pll_chain_end(const PllStream& f, int t, int steps, int last, bool demoted, float integ,
                                              float phase, unsigned long long resumed, unsigned long long run, int slot,
                                              unsigned long long n_redo, unsigned long long* stats, unsigned* redos) {
    const long long jf = steps * last;
    const unsigned long long n_dem = demoted ? (unsigned long long)(f.n - jf) : 0ull;
    const float a = (float)(f.pr_at(jf - 1) + (double)phase);
    PllState q;
    PllCtx c{};
    pll_state_at(q, c, integ, phase, f.trig0, jf, a, DeviceLib{});
    if (n_dem == 0) f.exact(q, c, jf, f.n);
    if (t == 0) {
        float* S = f.S;
        S[0] = q.integ; S[1] = q.phase; S[2] = q.fbI; S[3] = q.fbQ; S[5] = q.trig;
        S[6] = __builtin_bit_cast(float, (int)n_dem);
        if (stats) {
            atomicAdd(stats, resumed);
            atomicAdd(stats + 1, run);
        }
        if (redos) {
            atomicAdd(&redos[kPllRedoSlots * (size_t)f.s + slot], (unsigned)n_redo);
            atomicAdd(&redos[kPllRedoSlots * (size_t)f.s + 4 + slot], (unsigned)n_dem);
        }
    }
}

#ifdef FMRX_AB_PROF
// the "redos per stream" line of one form's per-stream counters (FMRX_AB_PROF's printers)
inline void prof_print_redos(const char* name, const unsigned int* rs, int n_streams) {
    unsigned long long tot = 0;
    unsigned int mx = 0;
    int n = 0, arg = -1;
    for (int k = 0; k < n_streams; k++) {
        tot += rs[k];
        if (rs[k]) n++;
        if (rs[k] > mx) { mx = rs[k]; arg = k; }
    }
    if (tot)
        std::fprintf(stderr, "redos per stream, %s: total %llu over %d streams, max %u (stream %d)\n", name, tot, n, mx,
                     arg);
}
#endif

// ---- host side: the launch of an index or count form (pll_idx.hip, pll_cnt.hip) ----------------
//
// A form's workgroup must be resident on one CU for its waves to run side by side (the chain
// spins on barriers with its evaluators): checked once per kernel against the compiled register
// and LDS use, so a build that outgrows it fails loudly instead of serialising.  -1: not resident,
// -2: the launch failed.
template <auto Kernel, int Threads>
int pll_runner_launch(const PllRunnerArgs& a, const PllForm& f) {
    static const int resident = [] {
        int nb = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kernel, Threads, 0) == hipSuccess ? nb : 0;
    }();
    if (resident < 1) return -1;
    hipLaunchKernelGGL(Kernel, dim3(a.n_streams), dim3(Threads), 0, a.s, a.io, a.n, a.n_streams, a.stride, a.step,
                       a.norm_bw, a.st, a.out, a.ostride, a.inject, a.miss, f.lo, f.hi, a.stats, a.redos);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace
}  // namespace fmrx
