// pll_idx.hip — pll_idx_kernel: the index runner of the predicted-trigArg PLL (src/filter.cpp:157-171),
// one stream a workgroup of 1 + NW waves, trigOffset in [2^17, 2^20).
//
// Below 2^20 trigArg's float grid (2^-8 .. 2^-5 rad) is finer than the phase moves in the two
// intervals between a prediction and its use, so three or five candidates miss; 16 to 64 do not
// (tools/pll_predict.cpp, profiles/r04/pll_predict_below_2_20.txt: 16-step intervals from the
// phase one interval back hit with 64 candidates on 0.9999+ of them in [2^17, 2^18), with 32 in
// [2^18, 2^19), with 16 in [2^19, 2^20); the [2^17, 2^18) form runs 32 (~0.99 of intervals hit,
// the misses redone: faster than 64 evaluations a step, profiles/r04/ab_idx17_nc32/)).  Compares
// against NC - 1 thresholds would cost the chain 2 (NC - 1) instructions a step, so here the chain forms the step's trigArg itself --
// float(P + (double)phase), filter.cpp:165, three instructions -- and turns it into a lane index:
// the NC candidates of a step c0 - NC/2 .. c0 + NC/2 - 1 sit in NC consecutive lanes of one VGPR
// row (64 / NC steps a row), so e = v_readlane(row, bits(trigArg) - base) with
// base = bits(c0) - NC/2 - the step's lane offset:
//   the chain (wave 0), per step: e from the previous trigArg's lane (v_readlane), (Ki e, Kp e),
//     the three float updates (filter.cpp:161-162), trigArg (cvt, add_f64, cvt), its lane index
//     (sub, v_readfirstlane), the index recorded in lane J of a row (v_writelane) -- 11 VALU a
//     step whatever NC is.  After the interval it tests the row (every index inside its step's
//     NC lanes) and the phase (not NaN: an uncertified candidate's e is NaN, so a chain that took
//     one carries NaN from there); a miss is redone on the exact path at once, from the state at
//     the interval's start (in registers), so it costs 16 exact steps and no pipeline restart: the
//     evaluators' next interval was predicted from the phase before the missed one, still right;
//   the evaluators (waves 1 .. NW, one SIMD each), per interval k: interval k + 1's candidate
//     rows (pred_e_cert for each lane's candidate, NaN where uncertified), P and base of each
//     step, from the phase at interval k's start; wave 1 also stores interval k - 1's trigArgs
//     (base + index: the candidate IS the trigArg) unless the chain redid it.
// So the runner is exact by construction, as pll_pipe_kernel: every e the chain used is a
// certified candidate's that is the true trigArg.  One launch runs a form's whole range of the
// call and leaves the exact end state in st.
#include "pll_runner.h"

namespace fmrx {

#ifdef FMRX_AB_PROF
__device__ unsigned long long g_idx_prof[6];
constexpr int kProfStreams = 4096;
__device__ unsigned int g_idx_redo_stream[kProfStreams];  // redos per stream (blockIdx.x)
#endif

namespace {

template <int NC, int NW>
__global__ void __launch_bounds__(64 * (1 + NW)) __attribute__((amdgpu_waves_per_eu(1, 1)))
pll_idx_kernel(const float* io, int n, int n_streams, size_t stride, double step, float norm_bw, float* st,
               float* out_base, size_t ostride, int inject, int miss, float lo, float hi, unsigned long long* stats,
               unsigned* redos) {
    constexpr int NI = 16;          // steps an interval
    constexpr int SPP = 64 / NC;    // steps a candidate row
    constexpr int NR = NI / SPP;    // candidate rows an interval
    constexpr int HC = NC / 2;      // candidates c0 - HC .. c0 + HC - 1
    constexpr int RD = 4;           // intervals of step inputs in flight
    constexpr int NP = (NR + NW - 1) / NW;  // rows an evaluator wave computes
    static_assert(NC == 16 || NC == 32 || NC == 64, "a power of two dividing the wave");
    // rings of four intervals (interval k in slot k & 3): per step (P lo, P hi, base, -) (sp), the
    // candidate rows (se), the chain's lane index of each step's trigArg (srow), its (integ,
    // phase) at the interval's end (sst), "redone exactly" (sexact)
    __shared__ float4 sp[4][NI];
    __shared__ float se[4][NR][64];
    __shared__ int srow[4][NI];
    __shared__ float4 sst[4];  // (integ, phase, the verdict "redone exactly" as int bits, -)
    __shared__ int sexact[4];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), t = threadIdx.x & 63;
    PllStream f;
    if (pll_stream_open(f, io, n, stride, step, norm_bw, st, out_base, ostride, redos)) return;
    const bool in_domain = pll_pipe_stream(f.p.trig, step, lo, hi);
    const int nb = n / NI;
    const int ni = nb;  // intervals 1 .. nb from the range's first step (the first predicted too)
    const int inj = pll_hook_inject(inject, f.s, ni);
    if (ni < 2 || !in_domain) {
        pll_stream_all_exact(f, w, t, in_domain, (unsigned long long)nb, stats);
        return;
    }
    auto j0 = [](int k) { return NI * (k - 1); };  // interval k's first step (k >= 1)

    if (w > 0) {
        // this wave's rows r = w - 1 + NW q; lane t: step J = r SPP + t / NC, candidate t % NC
        auto ld = [&](int k, float (&v)[NP]) {
            const int kk = k <= ni ? k : ni;
#pragma unroll
            for (int q = 0; q < NP; q++) {
                const int r = min(w - 1 + NW * q, NR - 1);
                const int j = j0(kk) + r * SPP + t / NC;
                v[q] = f.x[min(j + 1, n - 1)];  // the step the e is for
            }
        };
        auto put = [&](int k, float phase_ref, const float (&v)[NP]) {
            const int sl = k & 3;
#pragma unroll
            for (int q = 0; q < NP; q++) {
                const int r = w - 1 + NW * q;
                if (NP * NW > NR && r >= NR) break;
                const int J = r * SPP + t / NC, kc = t % NC;
                const int j = j0(k) + J;
                const double pr = f.pr_at(j);
                const uint32_t cb = __builtin_bit_cast(uint32_t, (float)(pr + (double)phase_ref));
                bool ok;
                const float e = pred_e_cert(__builtin_bit_cast(float, cb - (uint32_t)HC + (uint32_t)kc), v[q],
                                            pll_iv(v[q]), ok);
                // a candidate that is not a positive finite float never certifies: c0 < 2^126
                const bool fin = cb > (uint32_t)HC && cb < 0x7F000000u;
                se[sl][r][t] = ok && fin ? e : __builtin_nanf("");
                if (kc == 0) {
                    const uint64_t pb = __builtin_bit_cast(uint64_t, pr);
                    sp[sl][J] = make_float4(__builtin_bit_cast(float, (uint32_t)pb),
                                            __builtin_bit_cast(float, (uint32_t)(pb >> 32)),
                                            __builtin_bit_cast(float, cb - (uint32_t)HC - (uint32_t)(NC * (J % SPP))),
                                            0.0f);
                }
            }
        };
        // test hook pll_pipe_miss = -m (m >= 2): every interval from m - 1 on misses -- its step-0
        // base moved off the candidates, so the chain's lane index leaves the row (wave 1, lane 0)
        auto hook_poison = [&](int k) {
            if (miss <= -2 && k >= -miss - 1 && w == 1 && t == 0)
                reinterpret_cast<uint32_t*>(&sp[k & 3][0])[2] += 0x40000000u;
        };
        // wave 1: interval k's trigArgs, base + the chain's lane index (the chain stored a redone
        // interval itself)
        auto store = [&](int k) {
            if (w != 1) return;
            const int sl = k & 3;
            if (sexact[sl]) return;
            const int J = t & (NI - 1);
            const float a = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, sp[sl][J].z) + (uint32_t)srow[sl][J]);
            if (t < NI) f.out[j0(k) + J] = a;
        };
        float vq[RD][NP];
#pragma unroll
        for (int u = 0; u < RD; u++) ld(1 + u, vq[(1 + u) % RD]);
        put(1, f.p.phase, vq[1 % RD]);  // interval 1 from the start phase (its own start)
        hook_poison(1);
        ld(1 + RD, vq[1 % RD]);
        __syncthreads();  // (prologue)
        unsigned long long ev_body = 0, ev_wait = 0;
        // pll_demote is the chain's (its verdicts are at hand there, a few scalar ops an interval):
        // it may leave only after the last interval of one of these groups of RD, saying so in
        // that interval's state word (w); the evaluators look once a group, store that interval's
        // trigArgs and leave too, without another barrier (a test per interval cost the index forms
        // ~3 ns a step: the evaluators set their pace)
        bool left = false;
        for (int i0 = 1; i0 <= ni; i0 += RD) {
            unroll_ic(
                [&](auto uc) {
                    constexpr int u = decltype(uc)::value;
                    constexpr int sl = (2 + u) % RD;  // slot of interval i + 1
                    const int i = i0 + u;
                    if (i <= ni) {
                        const unsigned long long p0 = PROF_T();
                        // the chain's state at interval i's start
                        const float4 rs = sst[(i - 1) & 3];
                        if (i + 1 <= ni) {
                            put(i + 1, rs.y, vq[sl]);  // from the phase at interval i's start
                            hook_poison(i + 1);
                            ld(i + 1 + RD, vq[sl]);
                        }
                        store(i - 1);
                        const unsigned long long p1 = PROF_T();
                        __syncthreads();
                        ev_body += p1 - p0;
                        ev_wait += PROF_T() - p1;
                    }
                },
                std::make_integer_sequence<int, RD>{});
            // (at the group's end, not its start: a test skipped on the first group made LLVM peel
            // a whole group)
            if (!kAbNoDemote &&
                __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sst[(i0 + RD - 1) & 3].w)) != 0) {
                store(i0 + RD - 1);
                left = true;
                break;
            }
        }
        if (!left) store(ni);
        PROF_ADD(t == 0 && w == 1, g_idx_prof[2], ev_body);
        PROF_ADD(t == 0 && w == 1, g_idx_prof[3], ev_wait);
        return;
    }

    // ---- the chain
    float integ = f.p.integ, phase = f.p.phase;
    // the carry: the candidate row value of the previous trigArg and its lane (SGPR); after an
    // exact stretch that trigArg's exact e in every lane
    float cE = pll_chain_begin(f, t, sst, sexact);
    uint32_t cL = 0;
    auto carry_exact = [&](float a, int k) {
        cE = exact_e(a, f.x[min(j0(k), n - 1)]);
        cL = 0;
    };
    int dem_i = 0;  // the interval the chain left after (pll_chain_leaves)
    unsigned long long n_redo = 0, n_inj = 0, ch_body = 0, ch_wait = 0;
    const uint32_t off = (uint32_t)(NC * ((t & (NI - 1)) % SPP));  // lane t's step's lane offset
    // the last interval's verdict and pll_demote's history of them (SGPRs, pll_chain_leaves); the
    // start values are 0 but not constants to the compiler
    // (constants there made LLVM peel the first interval: a second copy of the chain loop)
    uint32_t prev_bad = n < 0 ? 1u : 0u, hist = n < 0 ? 1u : 0u;
    for (int i = 1; i <= ni; i++) {
        const unsigned long long p0 = PROF_T();
        const int is = i & 3;
        const float integ0 = integ, phase0 = phase;
        const bool leave = pll_chain_leaves<RD, NI, kPllDemoteMissesIdx>(hist, prev_bad, i, ni, n, integ, phase);
        // the interval's data before its steps (NI 16-byte broadcasts, NR row reads)
        float4 D[NI];
        float E[NR];
#pragma unroll
        for (int J = 0; J < NI; J++) D[J] = sp[is][J];
#pragma unroll
        for (int r = 0; r < NR; r++) E[r] = se[is][r][t];
        __builtin_amdgcn_sched_barrier(0);
        int row = 0;
        unroll_ic(
            [&](auto jc) {
                constexpr int J = decltype(jc)::value;
                // step J: e from the previous trigArg's candidate lane, filter.cpp:161-162
                const float e = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cE), cL));
                const float2v kv = float2v{f.Ki, f.Kp} * e;
                integ = integ + kv.x;
                phase = phase + (kv.y + integ);
                // trigArg (filter.cpp:165) and its lane in step J's candidate row
                const double P = __builtin_bit_cast(double, make_uint2(__builtin_bit_cast(uint32_t, D[J].x),
                                                                       __builtin_bit_cast(uint32_t, D[J].y)));
                const float a = (float)(P + (double)phase);
                cL = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, a) - __builtin_bit_cast(uint32_t, D[J].z));
                cE = E[J / SPP];
                int rw = row;  // (a local: clang rejects a captured variable as an asm operand here)
                const uint32_t sl = cL;
                asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(rw) : "s"(sl), "i"(J));
                row = rw;
            },
            std::make_integer_sequence<int, NI>{});
        // the interval's verdict: every trigArg's lane inside its step's candidates, no NaN e
        // taken (the phase), the start state in pll_batch_fast's range; test hooks force misses
        const bool lane_bad = t < NI && (uint32_t)row - off >= (uint32_t)NC;
        // (one ballot over the lane test and the uniform ones: provably uniform, an SGPR -- the redo
        // branch scalar and pll_demote's history SALU work, no readfirstlane round trip)
        const bool bad = __builtin_amdgcn_ballot_w64(lane_bad || !(phase == phase) ||
                                                     !(fabsf(phase0) < kPllMaxPhase && fabsf(integ0) < kPllMaxInteg)) != 0 ||
                         i == min(miss, ni) || i == inj;
        if (bad) {  // uniform: redo the interval exactly from its start (the chain stores it)
            n_redo++;
            n_inj += i == inj ? 1 : 0;
            carry_exact(pll_redo_interval(f, i, NI, integ0, phase0, integ, phase), i + 1);
        }
        if (t < NI) srow[is][t] = row;
        prev_bad = bad ? 1u : 0u;
        sst[is] = make_float4(integ, phase, __builtin_bit_cast(float, bad ? 1 : 0), __builtin_bit_cast(float, leave ? 1 : 0));
        sexact[is] = bad ? 1 : 0;
        const unsigned long long p1 = PROF_T();
        __syncthreads();
        ch_body += p1 - p0;
        ch_wait += PROF_T() - p1;
        if (leave) {  // (the evaluators leave after this interval's barrier too)
            dem_i = i;
            break;
        }
    }
    PROF_ADD(t == 0, g_idx_prof[0], ch_body);
    PROF_ADD(t == 0, g_idx_prof[1], ch_wait);
    PROF_ADD(t == 0, g_idx_prof[4], (unsigned long long)ni);
    PROF_ADD(t == 0, g_idx_prof[5], n_redo);
    PROF_ADD(t == 0 && f.s < kProfStreams, g_idx_redo_stream[f.s], (unsigned int)n_redo);
    // "resumed": the inject hook's forced redos only; fmrx_debug_pll_redos: slot 0, [2^17, 2^20)
    pll_chain_end(f, t, NI, dem_i ? dem_i : ni, dem_i != 0, integ, phase, n_inj, (unsigned long long)nb, 0, n_redo,
                  stats, redos);
}

}  // namespace

#ifdef FMRX_AB_PROF
static void print_idx_prof() {
    unsigned long long h[6] = {};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_idx_prof), sizeof h) == hipSuccess && h[4])
        std::fprintf(stderr, "pll_idx prof: intervals %llu chain body %.1f wait %.1f, evaluator body %.1f wait %.1f "
                     "(shader cycles per interval), %llu redos\n", h[4], (double)h[0] / h[4], (double)h[1] / h[4],
                     (double)h[2] / h[4], (double)h[3] / h[4], h[5]);
    static unsigned int rs[kProfStreams];
    if (hipMemcpyFromSymbol(rs, HIP_SYMBOL(g_idx_redo_stream), sizeof rs) == hipSuccess)
        prof_print_redos("index", rs, kProfStreams);
}
#endif

#ifndef FMRX_IDX17_NC
#define FMRX_IDX17_NC 32
#endif
#ifndef FMRX_IDX18_NC
#define FMRX_IDX18_NC 32
#endif
#ifndef FMRX_IDX_NW
#define FMRX_IDX_NW 4  // evaluator waves of the 32-candidate forms: two rows of candidates each
                       // (three waves: three rows, evaluator-bound; profiles/r04/ab_idx_nw4/)
#endif

int launch_pll_idx(const PllRunnerArgs& a, int form) {
#ifdef FMRX_AB_PROF
    [[maybe_unused]] static const int prof_reg = std::atexit(print_idx_prof);  // once
#endif
    if (a.n <= 0) return 0;
    const PllForm& f = pll_form(form, false);  // (the kernel's intervals are kPllBatch steps, as every index row's)
    if (form == 17) return pll_runner_launch<pll_idx_kernel<FMRX_IDX17_NC, FMRX_IDX_NW>, 64 * (1 + FMRX_IDX_NW)>(a, f);
    if (form == 18) return pll_runner_launch<pll_idx_kernel<FMRX_IDX18_NC, FMRX_IDX_NW>, 64 * (1 + FMRX_IDX_NW)>(a, f);
    return pll_runner_launch<pll_idx_kernel<16, 3>, 64 * (1 + 3)>(a, f);
}

}  // namespace fmrx
