// pll_pipe.hip — pll_pipe_kernel: the three-wave predicted-trigArg PLL runner (src/filter.cpp:157-171),
// one stream a workgroup of three waves, trigOffset from 2^20 on, the 2^24 stick included.
//
// pll_pred_kernel's chain wave issues ~16 VALU a step (the candidate choice, the updates, trigArg
// and its check), and one wave issues a VALU per ~4 cycles, dependent or not (tools/ubench_dep.hip,
// profiles/r03/ubench_dep.txt): its step costs its instruction count, wait states included.  Here
// the chain keeps only the recurrence -- the candidate choice (compares of the phase into SGPR
// masks, v_cndmask), (Ki e, Kp e), the three float updates: 9 instructions a step with NC = 3
// candidates, 12 with 5, four steps an asm block (chain4_3 / chain4_5) -- and hands one state a
// batch, (integ, phase) after its last step, to the other waves:
//   wave 1: interval k + 1's e for the NC candidates c0 - NC/2 .. c0 + NC/2 of every step, each
//           with its certification (pred_e_cert: the float roundings of the candidate's sin/cos
//           and of atan2 proven as in pll_batch_fast);
//   wave 2: interval k + 1's NC - 1 phase thresholds a step, c0's bits and P; and interval
//           k - 1 replayed batch by batch from those states, one lane group a batch (the chain's
//           arithmetic on the same data, so the same phases), its trigArgs float(P + phase)
//           (filter.cpp:165), their check against the candidates AND the certification of the
//           candidate each step took, and the output stores.
// So the runner is exact by construction: every e the chain used is the exact path's e (a
// certified candidate that is the true trigArg), every state it carries is the exact path's.  No
// pll_check_kernel, no resume kernel, no pre-pass (1/v and P = step x trigOffset are formed
// inline, pll_side's arithmetic): one launch runs a form's whole range of the call, however long,
// and leaves the exact end state in st.
// The candidates of interval k + 1 come from the phase at the start of interval k
// (tools/pll_predict.cpp, lookback 2).  NC = 3 with 64-step intervals from 2^22 (every interval
// of the bench stream hit), NC = 5 with 64-step intervals in [2^21, 2^22) (99.97 %) and with
// 16-step ones in [2^20, 2^21) (99.7 %).  The chain reads an interval's data in bursts before
// their steps (spread over the steps the reads stall it more: tools/ubench_chain.hip,
// profiles/r03/ubench_chain.txt).  A missed interval (a trigArg outside its candidates, or taken
// from an uncertified one) -- wave 2 flags it in the interval after the chain ran it, the chain
// reads the flag at the end of the next one -- is redone on the exact path with the two after it
// (pll_redo from the state at the interval's start, kept in the LDS ring); every wave takes two
// more barriers around that redo, and the evaluators redo the next interval from the corrected
// phase.
#include "pll_runner.h"

namespace fmrx {

#ifdef FMRX_AB_PROF
__device__ unsigned long long g_pipe_prof[6];
__device__ unsigned long long g_pipe_prof_w2[4];  // wave 2's body / barrier wait / put / check
__device__ unsigned long long g_miss_reason[3];   // pll_pipe_kernel's missed steps by reason
// redos per stream (blockIdx.x) and form: 16-step, 64-step five, three
constexpr int kProfStreams = 4096;
__device__ unsigned int g_pipe_redo_stream[3][kProfStreams];
#endif

namespace {

// pick (pll_runner.h) with five candidates: T = (T(c0 - 1), T(c0), T(c0 + 1), T(c0 + 2)), E =
// (e(c0 - 2) .. e(c0 + 1)), e2 = e(c0 + 2).  Four compares into SGPR masks, then four v_cndmask,
// each reading a mask written four VALU earlier (no wait state needed).
__device__ inline float pick5(float phase, float4 T, float4 E, float e2) {
    float e;
    uint64_t m0, m1, m2, m3;
    asm("v_cmp_ge_f32_e64 %1, %5, %6\n"
        "v_cmp_ge_f32_e64 %2, %5, %7\n"
        "v_cmp_ge_f32_e64 %3, %5, %8\n"
        "v_cmp_ge_f32_e64 %4, %5, %9\n"
        "v_cndmask_b32_e64 %0, %10, %11, %1\n"
        "v_cndmask_b32_e64 %0, %0, %12, %2\n"
        "v_cndmask_b32_e64 %0, %0, %13, %3\n"
        "v_cndmask_b32_e64 %0, %0, %14, %4"
        : "=&v"(e), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3)
        : "v"(phase), "v"(T.x), "v"(T.y), "v"(T.z), "v"(T.w), "v"(E.x), "v"(E.y), "v"(E.z), "v"(E.w), "v"(e2));
    return e;
}

// Four of pll_pipe_kernel's chain steps in one asm block: per step the candidate choice (pick /
// pick5), (Ki e, Kp e) as one v_pk_mul_f32 with (Ki, Kp) in an SGPR pair (kk: Ki low, Kp high),
// and the three float updates integ += Ki e, phase += Kp e + integ (filter.cpp:161-162), each
// product and sum rounded on its own as there.  9 instructions a step with three candidates, 12
// with five.  Compiled step by step, the same chain issued 11 and 14: the compiler puts a wait
// state after every asm statement whose result a VALU reads (it cannot see the statement's last
// instruction), and another after a v_pk_mul_f32 reading (Ki, Kp) from VGPRs; here one wait
// state follows each block of four (tools/ubench_chain.hip modes 9 and 20).  e and the two
// products live in v252-v255, clobbered.  ph[k] = the phase after step k.
#define FMRX_CHAIN_TAIL(P, Q)                                    \
    "v_pk_mul_f32 v[254:255], v[252:253], %[kk] op_sel_hi:[0,1]\n" \
    "v_add_f32 %[ig], %[ig], v254\n"                             \
    "v_add_f32 v255, v255, %[ig]\n"                              \
    "v_add_f32 " Q ", " P ", v255\n"
#define FMRX_CHAIN_STEP3(P, Q, K)                                      \
    "v_cmp_ge_f32_e64 %[m0], " P ", %[ta" #K "]\n"                       \
    "v_cmp_ge_f32_e64 %[m1], " P ", %[tb" #K "]\n"                       \
    "s_nop 0\n"                                                        \
    "v_cndmask_b32_e64 v252, %[ea" #K "], %[eb" #K "], %[m0]\n"          \
    "v_cndmask_b32_e64 v252, v252, %[ec" #K "], %[m1]\n" FMRX_CHAIN_TAIL(P, Q)
#define FMRX_CHAIN_STEP5(P, Q, K)                                      \
    "v_cmp_ge_f32_e64 %[m0], " P ", %[ta" #K "]\n"                       \
    "v_cmp_ge_f32_e64 %[m1], " P ", %[tb" #K "]\n"                       \
    "v_cmp_ge_f32_e64 %[m2], " P ", %[tc" #K "]\n"                       \
    "v_cmp_ge_f32_e64 %[m3], " P ", %[td" #K "]\n"                       \
    "v_cndmask_b32_e64 v252, %[ea" #K "], %[eb" #K "], %[m0]\n"          \
    "v_cndmask_b32_e64 v252, v252, %[ec" #K "], %[m1]\n"                 \
    "v_cndmask_b32_e64 v252, v252, %[ed" #K "], %[m2]\n"                 \
    "v_cndmask_b32_e64 v252, v252, %[ee" #K "], %[m3]\n" FMRX_CHAIN_TAIL(P, Q)
#define FMRX_CHAIN_OUTS \
    [q0] "=&v"(ph[0]), [q1] "=&v"(ph[1]), [q2] "=&v"(ph[2]), [q3] "=&v"(ph[3]), [ig] "+v"(integ)

// a[k] = (T0, T1, e(c0 - 1), e(c0)), ep[k] = e(c0 + 1) of step k (pick's arguments)
__device__ inline void chain4_3(float phase, float& integ, uint64_t kk, const float4 (&a)[4], const float (&ep)[4],
                                float (&ph)[4]) {
    uint64_t m0, m1;
    asm volatile(FMRX_CHAIN_STEP3("%[p]", "%[q0]", 0) FMRX_CHAIN_STEP3("%[q0]", "%[q1]", 1)
                     FMRX_CHAIN_STEP3("%[q1]", "%[q2]", 2) FMRX_CHAIN_STEP3("%[q2]", "%[q3]", 3)
                 : FMRX_CHAIN_OUTS, [m0] "=&s"(m0), [m1] "=&s"(m1)
                 : [p] "v"(phase), [kk] "s"(kk),
                   [ta0] "v"(a[0].x), [tb0] "v"(a[0].y), [ea0] "v"(a[0].z), [eb0] "v"(a[0].w), [ec0] "v"(ep[0]),
                   [ta1] "v"(a[1].x), [tb1] "v"(a[1].y), [ea1] "v"(a[1].z), [eb1] "v"(a[1].w), [ec1] "v"(ep[1]),
                   [ta2] "v"(a[2].x), [tb2] "v"(a[2].y), [ea2] "v"(a[2].z), [eb2] "v"(a[2].w), [ec2] "v"(ep[2]),
                   [ta3] "v"(a[3].x), [tb3] "v"(a[3].y), [ea3] "v"(a[3].z), [eb3] "v"(a[3].w), [ec3] "v"(ep[3])
                 : "v252", "v253", "v254", "v255");
}

// T[k], E[k], e2[k]: pick5's arguments of step k
__device__ inline void chain4_5(float phase, float& integ, uint64_t kk, const float4 (&T)[4], const float4 (&E)[4],
                                const float (&e2)[4], float (&ph)[4]) {
    uint64_t m0, m1, m2, m3;
    asm volatile(FMRX_CHAIN_STEP5("%[p]", "%[q0]", 0) FMRX_CHAIN_STEP5("%[q0]", "%[q1]", 1)
                     FMRX_CHAIN_STEP5("%[q1]", "%[q2]", 2) FMRX_CHAIN_STEP5("%[q2]", "%[q3]", 3)
                 : FMRX_CHAIN_OUTS, [m0] "=&s"(m0), [m1] "=&s"(m1), [m2] "=&s"(m2), [m3] "=&s"(m3)
                 : [p] "v"(phase), [kk] "s"(kk),
                   [ta0] "v"(T[0].x), [tb0] "v"(T[0].y), [tc0] "v"(T[0].z), [td0] "v"(T[0].w),
                   [ea0] "v"(E[0].x), [eb0] "v"(E[0].y), [ec0] "v"(E[0].z), [ed0] "v"(E[0].w), [ee0] "v"(e2[0]),
                   [ta1] "v"(T[1].x), [tb1] "v"(T[1].y), [tc1] "v"(T[1].z), [td1] "v"(T[1].w),
                   [ea1] "v"(E[1].x), [eb1] "v"(E[1].y), [ec1] "v"(E[1].z), [ed1] "v"(E[1].w), [ee1] "v"(e2[1]),
                   [ta2] "v"(T[2].x), [tb2] "v"(T[2].y), [tc2] "v"(T[2].z), [td2] "v"(T[2].w),
                   [ea2] "v"(E[2].x), [eb2] "v"(E[2].y), [ec2] "v"(E[2].z), [ed2] "v"(E[2].w), [ee2] "v"(e2[2]),
                   [ta3] "v"(T[3].x), [tb3] "v"(T[3].y), [tc3] "v"(T[3].z), [td3] "v"(T[3].w),
                   [ea3] "v"(E[3].x), [eb3] "v"(E[3].y), [ec3] "v"(E[3].z), [ed3] "v"(E[3].w), [ee3] "v"(e2[3])
                 : "v252", "v253", "v254", "v255");
}
#undef FMRX_CHAIN_OUTS
#undef FMRX_CHAIN_STEP5
#undef FMRX_CHAIN_STEP3
#undef FMRX_CHAIN_TAIL

// One wave a SIMD (amdgpu_waves_per_eu): the register budget is the chain's, so the scheduler
// keeps each burst of reads whole instead of threading it through the steps for occupancy.
// io / out: the stream's input and trigArg rows from the range's first sample (stride / ostride
// floats a stream), n samples; st: the state (read at the start, the exact end state written).
// WIDE (the short-call form, launch_pll_pipe form 24): the 16-step five-candidate form from 2^20 on,
// across the later forms' ranges and the stick (five candidates cover what three do there)
template <int NB, int BPI, int RD, int NC, bool STK = false, bool WIDE = false>
__global__ void __launch_bounds__(192) __attribute__((amdgpu_waves_per_eu(1, 1))) pll_pipe_kernel(const float* io, int n, int n_streams, size_t stride,
                                                      double step, float norm_bw, float* st, float* out_base,
                                                      size_t ostride, int inject, int miss,
                                                      unsigned long long* stats, unsigned* redos) {
    constexpr int NI = NB * BPI;
    static_assert(NI == 16 || NI == 32 || NI == 64 || (BPI > 1 && (NI == 128 || NI == 256)),
                  "the evaluators' lane map: 64 / NI lanes a step, or NI / 64 steps a lane");
    static_assert(NC == 3 || NC == 5, "three or five candidates");
    // STK: the stuck trigOffset (2^24, filter.cpp:165-166: 69.9 s into a stream).  Every step's
    // P is then the same, so c0 = float(P + phase_ref) and the two thresholds are the interval's
    // constants: wave 2 forms them once (sthr) and the e of the three candidates sit three floats a
    // step (sek) -- 0.75 16-byte reads a step for the chain instead of 1.25
    static_assert(!STK || (NC == 3 && BPI > 1), "the stick form is the three-candidate replay form");
    constexpr int NIL = NI > 64 ? 64 : NI;  // the evaluators' lane map: step l + NIL sp on lane l
    constexpr int SPL = NI / NIL;          // steps a lane (128-step intervals: two)
    constexpr int LPS = 64 / NIL;          // evaluator lanes a step
    constexpr int HC = NC / 2;    // candidates c0 - HC .. c0 + HC
    // the chain's steps a burst of reads (its registers hold a burst's data)
#ifndef FMRX_CHM
#define FMRX_CHM 32
#endif
    constexpr int CHM = FMRX_CHM;
    constexpr int CH = NC == 5 ? 16 : (NI < CHM ? NI : CHM);
    // rings of four intervals (interval k in slot k & 3; slot 0 holds the range's start state), per step: NC = 3:
    // the thresholds of c0 and c0 + 1 ulp and the e of c0 - 1 and c0 (sel), the e of c0 + 1
    // (sep); NC = 5: the thresholds of c0 - 1 .. c0 + 2 (sel), the e of c0 - 2 .. c0 + 1 (sel2),
    // of c0 + 2 (sep); bits(c0) - HC (scb), P (spr); the certification of each candidate's e
    // (scert, byte r for c0 - HC + r); the chain's (integ, phase) at the end of each batch (sst);
    // per interval the check's verdict (smiss) and "redone exactly" (sexact)
    __shared__ float4 sel[STK ? 1 : 4][STK ? 1 : NI];  // (the stick form: sthr and sek instead)
    __shared__ float4 sel2[NC == 5 ? 4 : 1][NC == 5 ? NI : 1];
    __shared__ float sep[STK ? 1 : 4][STK ? 1 : NI];
    __shared__ uint32_t scb[4][NI];
    __shared__ double spr[4][NI];
    __shared__ uint8_t scert[4][NI][8];
    __shared__ float2 sst[4][BPI];
    // one batch an interval (the 16-step form): the replay below would be as long as the chain's
    // own interval, so the chain hands over every phase instead (sph) and wave 2 checks those
    constexpr bool REPLAY = BPI > 1;
    __shared__ float sph[REPLAY ? 1 : 4][REPLAY ? 1 : NI];
    __shared__ int smiss[4], sexact[4];
    __shared__ int sdemote;  // the chain demoted the stream (pll_demote) at its redo
    __shared__ __attribute__((aligned(16))) float sek[STK ? 4 : 1][STK ? 3 * NI : 4];
    __shared__ float2 sthr[4];
    // the candidate data the chain and the replay select from at step J of ring slot sl: (T0, T1,
    // e(c0 - 1), e(c0)) and e(c0 + 1)
    auto cand = [&](int sl, int J) {
        if constexpr (STK) {
            const float2 T = sthr[sl];
            return make_float4(T.x, T.y, sek[STK ? sl : 0][STK ? 3 * J : 0], sek[STK ? sl : 0][STK ? 3 * J + 1 : 0]);
        } else {
            return sel[sl][J];
        }
    };
    auto cand_ep = [&](int sl, int J) {
        if constexpr (STK) return sek[STK ? sl : 0][STK ? 3 * J + 2 : 0];
        else return sep[sl][J];
    };
    // the wave (readfirstlane: uniform, so the waves' branches and loops are scalar)
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), t = threadIdx.x & 63, l = t & (NIL - 1), h = t / NIL;
    const int s = blockIdx.x;  // grid = n_streams
    const float* x = io + (size_t)s * stride;
    float* out = out_base + (size_t)s * ostride;
    float* S = st + 8 * (size_t)s;
    const float Kp = norm_bw * static_cast<float>(2.666);
    const float Ki = (norm_bw * norm_bw) * static_cast<float>(3.555);
    // the stream's state, uniform over the group (readfirstlane): the domain test below and every
    // branch and loop after it stay scalar
    auto uni = [](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); };
    PllState p{uni(S[0]), uni(S[1]), uni(S[2]), uni(S[3]), uni(S[5])};
    // demoted by an earlier runner launch of this call (pll_demote; state slot 6: the steps it left
    // to pll_demoted_kernel, int bits): this range is theirs too -- add it and leave (uniform)
    if (const int rem = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, S[6])); rem > 0) {
        if (threadIdx.x == 0) {
            S[6] = __builtin_bit_cast(float, rem + n);
            if (redos) atomicAdd(&redos[kPllRedoSlots * (size_t)s + 4 + pll_redo_range(p.trig)], (unsigned)n);
        }
        return;
    }
    // the variant's domain (uniform over the group): NC = 3 from 2^22; NC = 5 with 64-step
    // intervals in [2^21, 2^22), with 16-step ones in [2^20, 2^21)
    static_assert(!WIDE || (NC == 5 && BPI == 1 && !STK), "the wide form is the 16-step five-candidate one");
    const bool in_domain = STK ? pll_pipe_stream(p.trig, step, kPllTrigStick)
                         : WIDE ? pll_pipe_stream(p.trig, step, kPllPipeMinLow)
                         : NC == 3 ? pll_pipe_stream(p.trig, step, kPllPipeMin)
                                   : NI >= 64 ? pll_pipe_stream(p.trig, step, kPllPipeMin5, kPllPipeMin - 1.0f)
                                              : pll_pipe_stream(p.trig, step, kPllPipeMinLow, kPllPipeMin5 - 1.0f);
    const float trig0 = p.trig;
    const double t0d = (double)trig0;
    // pll_side's P of step j (trigOffset after the step's increment, stuck at 2^24)
    auto pr_at = [&](long long j) {
        return step * (double)(float)fmin(t0d + (double)(j + 1), (double)kPllTrigStick);
    };
    const int nb = n / NB;
    const int ni = nb / BPI;  // intervals 1 .. ni from the range's first step (the first predicted too)
    // test hook: a miss on interval 1 + (inject + s) % ni of this stream (the exact redo runs)
    const int inj = inject >= 0 && ni > 0 ? 1 + (inject + s) % ni : -1;
    // steps [j0, j1) exactly from state q (c): outputs
    auto exact = [&](PllState& q, PllCtx& c, long long j0, long long j1) {
        if (j1 > j0) {
            const PllPair z = pll_redo(q, c, x + j0, out + j0, (int)(j1 - j0), Ki, Kp, step, true);
            q = z.p;
            c = z.ctx;
        }
    };
    // a short range, or a stream outside the form's domain (the host's trigOffset bounds were
    // wrong: costs speed, never bits): every step exactly (no barrier is reached)
    if (ni < 2 || !in_domain) {
        if (w == 0) {
            PllCtx c{};
            c.valid = false;
            exact(p, c, 0, n);
            if (t == 0) {
                S[0] = p.integ; S[1] = p.phase; S[2] = p.fbI; S[3] = p.fbQ; S[5] = p.trig;
                S[6] = 0.0f;  // not demoted (pll_demoted_kernel)
                if (stats) {  // outside the domain: the whole range "resumed" on the exact path
                    if (!in_domain) atomicAdd(stats, (unsigned long long)nb);
                    atomicAdd(stats + 1, (unsigned long long)nb);
                }
            }
        }
        return;
    }
    auto j0 = [](int k) { return (k - 1) * NI; };  // interval k's first step (k >= 1)

    if (w > 0) {
        // ring of RD intervals of step inputs, interval k in slot k % RD, loaded RD - 1 ahead
        float vq[RD][SPL];
        auto ld = [&](int k, float (&v)[SPL]) {
#pragma unroll
            for (int sp = 0; sp < SPL; sp++) {
                const int j = j0(k <= ni ? k : ni) + l + NIL * sp;
                v[sp] = x[min(j + 1, n - 1)];  // the step the e is for
            }
        };
        // interval k's candidate data from phase_ref, the phase at the start of interval k - 1:
        // E1 lane (h, l) the e (and its certification) of candidates c0 - HC + r of step l, r = h,
        // h + LPS, ... < NC; E2 lane (h, l) the thresholds of c0 - HC + 1 + r, r = h, h + LPS,
        // ... < NC - 1, lanes h = 0 also c0's bits and P
        auto put = [&](int k, float phase_ref, const float (&vs)[SPL]) {
#pragma unroll
          for (int sp = 0; sp < SPL; sp++) {
            const int ls = l + NIL * sp;  // this lane's step
            const float v = vs[sp];
            const int j = j0(k <= ni ? k : ni) + ls;
            const double pr = pr_at(j);
            const float c0 = (float)(pr + (double)phase_ref);
            const uint32_t cb = __builtin_bit_cast(uint32_t, c0);
            const int sl = k & 3;
            if (w == 1) {
                const double iv = pll_iv(v);
                // one candidate at a time (unrolled, the five certified evaluations interleave and
                // spill the kernel's registers)
#pragma unroll 1
                for (int r = h; r < NC; r += LPS) {
                    bool ok;
                    const float e = pred_e_cert(__builtin_bit_cast(float, cb + (uint32_t)(r - HC)), v, iv, ok);
                    scert[sl][ls][r] = ok ? 1 : 0;
                    if (STK) sek[STK ? sl : 0][STK ? 3 * ls + r : 0] = e;
                    else if (r == NC - 1) sep[sl][ls] = e;
                    else if (NC == 3) reinterpret_cast<float*>(&sel[sl][ls])[2 + r] = e;
                    else reinterpret_cast<float*>(&sel2[NC == 5 ? sl : 0][NC == 5 ? ls : 0])[r] = e;
                }
                // the stick form's two thresholds, the interval's constants (every step's P and c0
                // are the same): here, where the evaluations leave time, not in wave 2 -- its check
                // sets the stick form's pace (profiles/r05/rprof_w2/)
                if (STK && t == 0 && sp == 0)
                    sthr[sl] = make_float2(phase_thr(pr, cb + (uint32_t)(1 - HC)), phase_thr(pr, cb + (uint32_t)(2 - HC)));
            } else {
                if (!STK) {
                    for (int r = h; r < NC - 1; r += LPS)
                        reinterpret_cast<float*>(&sel[sl][ls])[r] = phase_thr(pr, cb + (uint32_t)(r + 1 - HC));
                }
                if (h == 0) {
                    scb[sl][ls] = cb - (uint32_t)HC;
                    spr[sl][ls] = pr;
                }
            }
          }
        };
        // E2: interval k's check.  Lane group g = t / NB replays batch g of the interval (BPI
        // batches) from the chain's state before it -- the chain's steps on the same candidate data,
        // so the same phases -- forms each step's trigArg float(P + phase) (filter.cpp:165) and
        // checks it against the step's candidates and that candidate's certification; lane l of
        // the group stores step l's.  A candidate that is not a positive finite float, a
        // threshold outside its window (-inf), an uncertified e or a state out of pll_batch_fast's
        // range counts as a miss.  (The chain hands over one state a batch instead of every phase:
        // an LDS store of four phases cost it ~20 cycles.)
        auto verdict = [&](int sl, int J, float a) {
            const uint32_t cm = scb[sl][J];
            const float4 tt = cand(sl, J);
            const float c0 = __builtin_bit_cast(float, cm + (uint32_t)HC);
            const bool thr_ok = tt.x > -__builtin_inff() && tt.y > -__builtin_inff() &&
                                (NC == 3 || (tt.z > -__builtin_inff() && tt.w > -__builtin_inff()));
            const uint32_t idx = __builtin_bit_cast(uint32_t, a) - cm;
            const bool cert = idx < (uint32_t)NC && scert[sl][J][idx < (uint32_t)NC ? idx : 0] != 0;
#ifdef FMRX_AB_PROF
            // why a step misses: its trigArg outside the candidates / its e uncertified / a threshold
            // outside its window
            if (idx >= (uint32_t)NC) atomicAdd(&g_miss_reason[0], 1ull);
            else if (!cert) atomicAdd(&g_miss_reason[1], 1ull);
            if (!thr_ok) atomicAdd(&g_miss_reason[2], 1ull);
#endif
            return !cert || !thr_ok || !(c0 > 0.0f && c0 < 3.0e38f);
        };
        auto check = [&](int k) {
            if (w != 2) return;
            const int sl = k & 3;
            if (sexact[sl]) {  // redone exactly: the chain stored it
                if (t == 0) smiss[sl] = 0;
                return;
            }
            if constexpr (!REPLAY) {  // the chain's phases, lanes h = 0
                const float ph = sph[REPLAY ? 0 : sl][REPLAY ? 0 : l];
                const float a = (float)(spr[sl][l] + (double)ph);
                if (h == 0) out[j0(k) + l] = a;
                // pll_batch_fast's range test, on the state at the batch's start
                const float2 r0 = sst[(k - 1) & 3][BPI - 1];
                const bool bad = verdict(sl, l, a) || !(fabsf(r0.y) < kPllMaxPhase && fabsf(r0.x) < kPllMaxInteg);
                const bool any = __builtin_amdgcn_ballot_w64(h == 0 && bad) != 0 || pll_hook_miss(k, miss, ni);
                // test hooks: a forced miss (the redo path); inject's is counted as resumed
                if (t == 0) smiss[sl] = k == inj ? 2 : any ? 1 : 0;
                return;
            }
            // 64 / NB lane groups a wave, so BPI > 64 / NB batches (128-step intervals) take rounds
            constexpr int GPW = 64 / NB, RND = (BPI + GPW - 1) / GPW;
            const int g0 = t / NB, lg = t & (NB - 1);
            bool anybad = false;
#pragma unroll 1
            for (int rd = 0; rd < RND; rd++) {
                const int g = g0 + GPW * rd;
                const bool act = g < BPI;
                const int gb = act ? g : 0;  // the groups past the interval's batches replay batch 0
                const float2 r0 = gb > 0 ? sst[sl][gb - 1] : sst[(k - 1) & 3][BPI - 1];
                float ig = r0.x, ph = r0.y;
                // step 0's candidate data: those of the trigArg before it (after an exactly redone
                // interval that trigArg's exact e in every slot, as the chain's carry)
                float4 ca, ca2;
                float cep;
                if (gb > 0) {
                    ca = cand(sl, NB * gb - 1);
                    cep = cand_ep(sl, NB * gb - 1);
                    ca2 = sel2[NC == 5 ? sl : 0][NC == 5 ? NB * gb - 1 : 0];
                } else if (sexact[(k - 1) & 3]) {
                    const int j = j0(k);
                    // (interval 1: the range's first step, from the state's own feedback)
                    const float e = k == 1 ? exact_e_fb(p.fbI, p.fbQ, x[0])
                                           : exact_e((float)(pr_at(j - 1) + (double)ph), x[min(j, n - 1)]);
                    ca = NC == 3 ? make_float4(0.0f, 0.0f, e, e) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    ca2 = make_float4(e, e, e, e);
                    cep = e;
                } else {
                    ca = cand((k - 1) & 3, NI - 1);
                    cep = cand_ep((k - 1) & 3, NI - 1);
                    ca2 = sel2[NC == 5 ? (k - 1) & 3 : 0][NC == 5 ? NI - 1 : 0];
                }
                // the batch's candidate data, read before the steps (the step loop then never waits on
                // LDS); lane l keeps the phase of step l and checks its own trigArg afterwards
                float4 da[NB], da2[NC == 5 ? NB : 1];
                float dep[NB];
                if constexpr (STK) {  // the batch's three e a step as 16-byte reads, the thresholds once
                    const float2 T = sthr[sl];
                    float ek[3 * NB];
#pragma unroll
                    for (int q = 0; q < 3 * NB / 4; q++)
                        *reinterpret_cast<float4*>(&ek[4 * q]) =
                            reinterpret_cast<const float4*>(&sek[STK ? sl : 0][STK ? 3 * NB * gb : 0])[q];
#pragma unroll
                    for (int j = 0; j < NB - 1; j++) {
                        da[j] = make_float4(T.x, T.y, ek[3 * j], ek[3 * j + 1]);
                        dep[j] = ek[3 * j + 2];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < NB - 1; j++) {
                        da[j] = cand(sl, NB * gb + j);
                        dep[j] = cand_ep(sl, NB * gb + j);
                        if constexpr (NC == 5) da2[j] = sel2[NC == 5 ? sl : 0][NC == 5 ? NB * gb + j : 0];
                    }
                }
                // pll_batch_fast's range test, on the state at the batch's start
                const bool range_ok = fabsf(r0.y) < kPllMaxPhase && fabsf(r0.x) < kPllMaxInteg;
                float mine = 0.0f;
#pragma unroll
                for (int j = 0; j < NB; j++) {
                    const float e = NC == 3 ? pick(ph, j == 0 ? ca : da[j > 0 ? j - 1 : 0], j == 0 ? cep : dep[j > 0 ? j - 1 : 0])
                                            : pick5(ph, j == 0 ? ca : da[j > 0 ? j - 1 : 0], j == 0 ? ca2 : da2[NC == 5 && j > 0 ? j - 1 : 0],
                                                    j == 0 ? cep : dep[j > 0 ? j - 1 : 0]);
                    const float2v kv = float2v{Ki, Kp} * e;
                    ig = ig + kv.x;
                    ph = ph + (kv.y + ig);
                    if (j == lg) mine = ph;
                }
                const int J = NB * gb + lg;  // this lane's step
                const float a = (float)(spr[sl][J] + (double)mine);
                const bool bad = verdict(sl, J, a) || !range_ok;
                if (act) out[j0(k) + J] = a;
                anybad = anybad || (act && bad);
            }
            const bool any = __builtin_amdgcn_ballot_w64(anybad) != 0 || pll_hook_miss(k, miss, ni);
            // test hooks: a forced miss (the redo path); inject's is counted as resumed
            if (t == 0) smiss[sl] = k == inj ? 2 : any ? 1 : 0;
        };
#pragma unroll
        for (int u = 0; u < RD; u++) ld(1 + u, vq[(1 + u) % RD]);
        put(1, p.phase, vq[1 % RD]);  // interval 1 from the initial phase
        ld(1 + RD, vq[1 % RD]);
        __syncthreads();  // (prologue)
        unsigned long long ev_body = 0, ev_wait = 0, ev_put = 0, ev_check = 0;
        // the chain demoted the stream at a redo (pll_demote): it runs the rest of the range alone
        bool demoted = false;
        // interval i: interval i + 1's data, interval i - 1's check; groups of RD intervals from
        // i0 = 1 (mod RD), so the ring slots are compile-time
        for (int i0 = 1; i0 <= ni && !demoted; i0 += RD) {
            unroll_ic(
                [&](auto uc) {
                    constexpr int u = decltype(uc)::value;
                    constexpr int sl = (2 + u) % RD;  // slot of interval i + 1
                    const int i = i0 + u;
                    if (i <= ni && !demoted) {
                        const unsigned long long p0 = PROF_T();
                        if (i + 1 <= ni) {
                            put(i + 1, sst[(i - 1) & 3][BPI - 1].y, vq[sl]);
                            ld(i + 1 + RD, vq[sl]);
                        }
                        const unsigned long long pa = PROF_T();
                        check(i - 1);
                        ev_put += pa - p0;
                        ev_check += PROF_T() - pa;
                        const int redo = __builtin_amdgcn_readfirstlane(smiss[(i - 2) & 3]);
                        if (redo) {
                            // the chain redoes interval i - 2 exactly, then runs i - 1 again on
                            // its candidates (from the phase at i - 2's start, which was right)
                            // and i on candidates predicted anew here from the corrected phase
                            __syncthreads();  // B1: the chain's exact redo of i - 2 follows
                            __syncthreads();  // B1.5: i - 2's exact end state is in the ring
                            if (__builtin_amdgcn_readfirstlane(sdemote)) {  // set before B1.5
                                demoted = true;
                                return;
                            }
                            {
                                float v[SPL];
                                ld(i, v);
                                put(i, sst[(i - 2) & 3][BPI - 1].y, v);
                            }
                            __syncthreads();  // B2: the chain ran i - 1 again
                            check(i - 1);
                            if (i + 1 <= ni) {  // interval i + 1 from the phase at i's start
                                float v[SPL];
                                ld(i + 1, v);
                                put(i + 1, sst[(i - 1) & 3][BPI - 1].y, v);
                            }
                            __syncthreads();  // B3: the chain ran i again
                        }
                        const unsigned long long p1 = PROF_T();
                        __syncthreads();
                        ev_body += p1 - p0;
                        ev_wait += PROF_T() - p1;
                    }
                },
                std::make_integer_sequence<int, RD>{});
        }
        if (!demoted) {
            check(ni);
            __syncthreads();  // the chain reads the last two verdicts
        }
        PROF_ADD(t == 0 && w == 1, g_pipe_prof[2], ev_body);
        PROF_ADD(t == 0 && w == 1, g_pipe_prof[3], ev_wait);
        PROF_ADD(t == 0 && w == 2, g_pipe_prof_w2[0], ev_body);
        PROF_ADD(t == 0 && w == 2, g_pipe_prof_w2[1], ev_wait);
        PROF_ADD(t == 0 && w == 2, g_pipe_prof_w2[2], ev_put);
        PROF_ADD(t == 0 && w == 2, g_pipe_prof_w2[3], ev_check);
        return;
    }

    // ---- the chain
    // interval 1 starts at the range's first step, predicted from the start phase like every other
    // (until round 6 its first batch ran on the exact path: 16 steps at ~400 ns, ~6 us a launch)
    float integ = p.integ, phase = p.phase;
    // (Ki, Kp) as an SGPR pair for the chain's v_pk_mul_f32 (uniform: readfirstlane)
    const uint64_t kk = (uint64_t)__builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, Ki)) |
                        ((uint64_t)__builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, Kp)) << 32);
    // the carry: step 0's candidate data (those of the previous interval's last trigArg); after
    // an exact stretch that trigArg's exact e in every slot
    float4 carry, carry2;
    float carry_ep;
    auto carry_exact = [&](float a, int k) {
        const float e = exact_e(a, x[min(j0(k), n - 1)]);
        carry = NC == 3 ? make_float4(0.0f, 0.0f, e, e) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        carry2 = make_float4(e, e, e, e);
        carry_ep = e;
    };
    {  // step 0's e from the state's feedback (the exact path's first step)
        const float e = exact_e_fb(p.fbI, p.fbQ, x[0]);
        carry = NC == 3 ? make_float4(0.0f, 0.0f, e, e) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        carry2 = make_float4(e, e, e, e);
        carry_ep = e;
    }
    if (t == 0) {
        sst[0][BPI - 1] = make_float2(integ, phase);  // the start of interval 1 (the evaluators' interval 2)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            smiss[k] = 0;
            sexact[k] = k == 0;
        }
        sdemote = 0;
    }
    __syncthreads();  // (prologue)
    unsigned long long ch_body = 0, ch_wait = 0, n_redo = 0, n_inj = 0, n_dem = 0;
    uint32_t hist = 0;  // the last 32 verdicts (pll_demote)
    bool demoted = false;
    PllState qd;        // demoted: the exact state at the end of the redone interval, and its step
    PllCtx cd{};
    long long jd = 0;
    // the exact state before interval f from the ring (its trigArg's sin / cos recomputed); before
    // interval 1 the range's start state as given (its feedback may not be that sin / cos: a state
    // set by the caller)
    auto state_before = [&](int f, PllState& q, PllCtx& c) {
        if (f <= 1) {
            q = p;
            c = PllCtx{};
            c.valid = false;
            return;
        }
        const float2 r0 = sst[(f - 1) & 3][BPI - 1];
        const float a = (float)(pr_at(j0(f) - 1) + (double)r0.y);  // the trigArg before it
        pll_state_at(q, c, r0.x, r0.y, trig0, (long long)j0(f), a, DeviceLib{});
    };
    // interval i on the fast chain from (integ, phase) and the carry, its data in ring slot i & 3
    auto run = [&](int i) {
        const int is = i & 3;
        // in bursts of CH steps: the data, 1.25 CH (NC = 5: 2.25 CH) 16-byte reads at once in the
        // order the steps need them (spread over the steps they stall the chain more,
        // tools/ubench_chain.hip), then the steps, then the batch states
        float4 A[CH], A2[NC == 5 ? CH : 1];
        float EP[CH];
        unroll_ic(
            [&](auto hc) {
                constexpr int H = decltype(hc)::value;
                if constexpr (STK) {  // three 16-byte reads a group of four steps, the thresholds once
                    const float2 T = sthr[is];
#pragma unroll
                    for (int q = 0; q < CH / 4; q++) {
                        float ek[12];
#pragma unroll
                        for (int u = 0; u < 3; u++)
                            *reinterpret_cast<float4*>(&ek[4 * u]) =
                                reinterpret_cast<const float4*>(&sek[STK ? is : 0][STK ? 3 * H * CH : 0])[3 * q + u];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            A[4 * q + u] = make_float4(T.x, T.y, ek[3 * u], ek[3 * u + 1]);
                            EP[4 * q + u] = ek[3 * u + 2];
                        }
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < CH / 4; q++) {
                        *reinterpret_cast<float4*>(&EP[4 * q]) = reinterpret_cast<const float4*>(&sep[is][H * CH])[q];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            A[4 * q + u] = sel[is][H * CH + 4 * q + u];
                            if constexpr (NC == 5) A2[4 * q + u] = sel2[NC == 5 ? is : 0][NC == 5 ? H * CH + 4 * q + u : 0];
                        }
                    }
                }
                float2 brec[CH / NB];  // (integ, phase) at the end of each batch of the burst
                float PH[REPLAY ? 1 : CH];  // (the 16-step form) the burst's phases
                unroll_ic(
                    [&](auto gc) {
                        constexpr int J = 4 * decltype(gc)::value;  // steps J .. J + 3
                        float4 a[4], a2[4];
                        float ep[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            a[u] = J + u == 0 ? carry : A[J + u > 0 ? J + u - 1 : 0];
                            ep[u] = J + u == 0 ? carry_ep : EP[J + u > 0 ? J + u - 1 : 0];
                            if constexpr (NC == 5) a2[u] = J + u == 0 ? carry2 : A2[J + u > 0 ? J + u - 1 : 0];
                        }
                        float q[4];
                        if constexpr (NC == 3)
                            chain4_3(phase, integ, kk, a, ep, q);
                        else
                            chain4_5(phase, integ, kk, a, a2, ep, q);
                        phase = q[3];
                        if constexpr (!REPLAY) {
#pragma unroll
                            for (int u = 0; u < 4; u++) PH[REPLAY ? 0 : J + u] = q[u];
                        }
                        if constexpr ((J + 3) % NB == NB - 1) brec[(J + 3) / NB] = make_float2(integ, phase);
                    },
                    std::make_integer_sequence<int, CH / 4>{});
                // Every read of the burst has landed by now (the steps used them), but the waitcnt
                // pass cannot tell: after the stores' exec-masked branch it would wait for the
                // stores too (lgkmcnt(0)) before the next burst's first use.  Waiting here is free.
                // (sched_barrier: the wait stays after the steps; the scheduler moves a bare
                // s_waitcnt up among the burst's first steps)
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
                __builtin_amdgcn_sched_barrier(0);
                // every lane stores (the chain's values are uniform: the same LDS words, the same
                // arithmetic), so no lane test on the chain -- its lane id was spilled to scratch
                // and reloaded at every burst
                if constexpr (!REPLAY) {
#pragma unroll
                    for (int q = 0; q < CH / 4; q++)
                        reinterpret_cast<float4*>(&sph[REPLAY ? 0 : is][REPLAY ? 0 : H * CH])[q] =
                            *reinterpret_cast<const float4*>(&PH[REPLAY ? 0 : 4 * q]);
                }
#pragma unroll
                for (int q = 0; q < CH / NB; q++) sst[is][H * (CH / NB) + q] = brec[q];
                carry = A[CH - 1];
                if constexpr (NC == 5) carry2 = A2[CH - 1];
                carry_ep = EP[CH - 1];
            },
            std::make_integer_sequence<int, NI / CH>{});
        sexact[is] = 0;
    };
    for (int i = 1; i <= ni; i++) {
        const unsigned long long p0 = PROF_T();
        const int flag = smiss[(i - 2) & 3];  // the verdict on interval i - 2 (slot 3 is clear at i = 1)
        run(i);
        const bool over = pll_demote(hist, __builtin_amdgcn_readfirstlane(flag) != 0);
        if (__builtin_amdgcn_readfirstlane(flag)) {
            n_redo++;
            n_inj += inj == i - 2 ? 1 : 0;  // the inject hook's interval, redone exactly
            __syncthreads();  // B1: E2's stores of interval i - 1 happen before the redo's
            // interval i - 2 (missed) exactly, from the state at its start (the end of interval
            // i - 3 in the ring; interval 1: the range's own start state, slot 0)
            const int f = i - 2;
            PllState q;
            PllCtx c{};
            state_before(f, q, c);
            exact(q, c, j0(f), j0(f) + NI);
            if (t == 0) {
                sst[f & 3][BPI - 1] = make_float2(q.integ, q.phase);
                sexact[f & 3] = 1;
                smiss[(i - 1) & 3] = 0;  // E2's verdict on the wrong interval i - 1
            }
            integ = q.integ;
            phase = q.phase;
            if (over && n >= kPllDemoteMinIntervals * NI &&  // demoted: the evaluators leave after B1.5,
                __builtin_amdgcn_ballot_w64(fabsf(q.phase) < kPllMaxPhase && fabsf(q.integ) < kPllMaxInteg) != 0) {
                                                               // pll_demoted_kernel runs the rest
                sdemote = 1;
                __syncthreads();  // B1.5
                demoted = true;
                qd = q;
                cd = c;
                jd = j0(f) + NI;
                break;
            }
            carry_exact((float)c.x, f + 1);
            __syncthreads();  // B1.5: the evaluators predict interval i anew from i - 2's end
            // interval i - 1 again on the fast chain: its candidates came from the phase at the
            // start of i - 2, which was right; E2 checks it again after B2
            run(i - 1);
            __syncthreads();  // B2: interval i's new candidates are in; E2 checks i - 1, the
                              // evaluators predict i + 1 from i - 1's end
            run(i);
            __syncthreads();  // B3
        }
        const unsigned long long p1 = PROF_T();
        __syncthreads();
        ch_body += p1 - p0;
        ch_wait += PROF_T() - p1;
    }
    PllState q;
    PllCtx c{};
    int f;  // the first interval the tail below runs exactly
    if (demoted) {  // the redone interval's exact end: pll_demoted_kernel runs the rest
        q = qd;
        c = cd;
        f = (int)(jd / NI) + 1;
        n_dem = (unsigned long long)(n - jd);
    } else {
        __syncthreads();  // E2's checks of the last two intervals
        // a miss in them: from the first missed interval on exactly; then the steps past the last
        // interval exactly, from the state at the end of the last good interval
        f = smiss[(ni - 1) & 3] ? ni - 1 : (smiss[ni & 3] ? ni : ni + 1);
        state_before(f, q, c);
        exact(q, c, j0(f), n);
    }
    if (t == 0) {
        S[0] = q.integ; S[1] = q.phase; S[2] = q.fbI; S[3] = q.fbQ; S[5] = q.trig;
        S[6] = __builtin_bit_cast(float, demoted ? (int)(n - jd) : 0);  // the steps left to pll_demoted_kernel, or 0
        // fmrx_debug_pll_stats: batches run; "resumed" only for the inject hook's forced redos
        // (the runner is exact by construction: its own redos of missed intervals are internal)
        if (stats) {
            const int fin = inj >= f ? 1 : 0;  // the hook's interval redone after the loop
            atomicAdd(stats, (n_inj + (unsigned long long)fin) * 3 * BPI);
            atomicAdd(stats + 1, (unsigned long long)nb);
        }
        // fmrx_debug_pll_redos: this stream's redone intervals and demoted steps
        if (redos) {  // by the range's trigOffset at its start (the wide 16-step form runs in any
                      // range from 2^20: launch_pll's short calls and long forms' tails)
            const int rg = pll_redo_range(trig0);
            atomicAdd(&redos[kPllRedoSlots * (size_t)s + rg], (unsigned)n_redo);
            atomicAdd(&redos[kPllRedoSlots * (size_t)s + 4 + rg], (unsigned)n_dem);
        }
    }
    PROF_ADD(t == 0, g_pipe_prof[0], ch_body);
    PROF_ADD(t == 0, g_pipe_prof[1], ch_wait);
    PROF_ADD(t == 0, g_pipe_prof[4], (unsigned long long)ni);
    PROF_ADD(t == 0, g_pipe_prof[5], n_redo);
    PROF_ADD(t == 0 && s < kProfStreams, g_pipe_redo_stream[NI == 16 ? 0 : NC == 5 ? 1 : 2][s], (unsigned int)n_redo);
}

}  // namespace

#ifdef FMRX_AB_PROF
static void print_pipe_prof() {
    unsigned long long h[6] = {};
    static unsigned int rs[3][kProfStreams];
    if (hipMemcpyFromSymbol(rs, HIP_SYMBOL(g_pipe_redo_stream), sizeof rs) == hipSuccess) {
        const char* names[3] = {"pipe 16-step", "pipe 64-step five", "pipe three"};
        for (int f = 0; f < 3; f++) prof_print_redos(names[f], rs[f], kProfStreams);
    }
    unsigned long long mr[3] = {};
    if (hipMemcpyFromSymbol(mr, HIP_SYMBOL(g_miss_reason), sizeof mr) == hipSuccess && (mr[0] | mr[1] | mr[2]))
        std::fprintf(stderr, "pll_pipe missed steps: trigArg outside the candidates %llu, e uncertified %llu, "
                     "threshold outside its window %llu\n", mr[0], mr[1], mr[2]);
    unsigned long long h2[4] = {};
    (void)hipMemcpyFromSymbol(h2, HIP_SYMBOL(g_pipe_prof_w2), sizeof h2);
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_pipe_prof), sizeof h) == hipSuccess && h[4]) {
        std::fprintf(stderr, "pll_pipe prof: wave 2 body %.1f wait %.1f, of the body its data %.1f and its check %.1f "
                     "(shader cycles per interval)\n", (double)h2[0] / h[4], (double)h2[1] / h[4], (double)h2[2] / h[4],
                     (double)h2[3] / h[4]);
        std::fprintf(stderr, "pll_pipe prof: intervals %llu chain body %.1f wait %.1f, evaluator body %.1f wait %.1f "
                     "(shader cycles per interval), %llu redos\n", h[4], (double)h[0] / h[4], (double)h[1] / h[4],
                     (double)h[2] / h[4], (double)h[3] / h[4], h[5]);
    }
}
#endif

#ifndef FMRX_PIPE_RD
#define FMRX_PIPE_RD 8  // intervals of step inputs in flight (the evaluators' loop is unrolled by it)
#endif
// One launch of a form's kernel: a stream a workgroup of three waves
template <auto Kernel>
static void pipe_launch(const PllRunnerArgs& a) {
    hipLaunchKernelGGL(Kernel, dim3(a.n_streams), dim3(192), 0, a.s, a.io, a.n, a.n_streams, a.stride, a.step, a.norm_bw,
                       a.st, a.out, a.ostride, a.inject, a.miss, a.stats, a.redos);
}

void launch_pll_pipe(const PllRunnerArgs& a, int form) {
#ifdef FMRX_AB_PROF
    [[maybe_unused]] static const int prof_reg = std::atexit(print_pipe_prof);  // once
#endif
    if (a.n <= 0) return;
    // kPllForms' interval of the form, in batches: the kernel's BPI
    constexpr auto bpi = [](int f) { return pll_form(f, false).interval / kPllBatch; };
    static_assert(bpi(25) == FMRX_PIPE25_BPI && bpi(24) == 1 && bpi(23) == FMRX_STICK_BPI &&
                      bpi(22) == FMRX_PIPE22_BPI && bpi(21) == FMRX_PIPE21_BPI && bpi(20) == 1,
                  "the instantiations below run pll_forms.h's intervals");
    constexpr int B = kPllBatch, RD = FMRX_PIPE_RD;
    if (form == 25)  // short calls from 2^22: three candidates in 128-step intervals (640 = 5 of them)
        pipe_launch<pll_pipe_kernel<B, FMRX_PIPE25_BPI, RD, 3>>(a);
    else if (form == 24)  // the short-call form: any trigOffset from 2^20, 16-step intervals
        pipe_launch<pll_pipe_kernel<B, 1, RD, 5, false, true>>(a);
    else if (form == 23)
        pipe_launch<pll_pipe_kernel<B, FMRX_STICK_BPI, RD, 3, true>>(a);
    else if (form == 22)
        pipe_launch<pll_pipe_kernel<B, FMRX_PIPE22_BPI, RD, 3>>(a);
    else if (form == 21)
        pipe_launch<pll_pipe_kernel<B, FMRX_PIPE21_BPI, RD, 5>>(a);
    else
        pipe_launch<pll_pipe_kernel<B, 1, RD, 5>>(a);
}

}  // namespace fmrx
