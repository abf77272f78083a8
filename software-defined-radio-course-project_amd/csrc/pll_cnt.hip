// pll_cnt.hip — pll_cnt_kernel: the count runner of the predicted-trigArg PLL (src/filter.cpp:157-171),
// one stream a workgroup of 1 + NW waves; the chain picks e by a count.
//
// The exact phase threshold of every candidate (phase_thr_exact: "trigArg >= c" is "phase >=
// T(c)", trigArg = float(P + (double)phase) being monotone in the float phase, filter.cpp:165)
// turns the candidate choice into ONE compare of the phase against a row of thresholds: lane l of
// step J's T row holds T(c_base + l) (l <= NC; +inf beyond), so the bits of the compare's mask
// are a prefix and their count is the trigArg's place in the window, plus one.  Lane l of the E
// row holds the e of candidate c_base + l - 1 (certified, NaN where not; lanes 0 and NC + 1 NaN:
// a trigArg below or above the window), so e = v_readlane(E, count) -- a compare, s_bcnt1 and a
// v_readlane whatever NC is (tools/ubench_cnt.hip mode 3: 60 cycles a step with the data in
// registers, against 91 for the index runner's f64 trigArg and lane index, mode 0).  So the
// window can be wide enough that a trigArg outside it is rare even for 64-step intervals
// predicted 64 to 128 steps ahead (tools/pll_predict.cpp, profiles/r04/g5/predict.txt).
//   the chain (wave 0), per step: e, (Ki e, Kp e), the three float updates (filter.cpp:161-162),
//     the compare and count, the count recorded in lane J of a row.  After the interval: a NaN
//     phase or carry e (a trigArg outside its window, an uncertified candidate) or a start state
//     out of the certified range redoes the interval on the exact path at once, from the state at
//     its start (the evaluators' next interval came from that state: no restart);
//   the evaluators (waves 1 .. NW), per interval k: interval k + 1's T and E rows from the phase
//     at interval k's start (c0 = float(P + phase_ref), c_base = c0 - NC / 2), items spread over
//     all their lanes; wave 1 also stores interval k - 1's trigArgs (c_base + count - 1: the
//     candidate IS the trigArg) unless the chain redid it.
// Exact by construction as pll_pipe_kernel / pll_idx_kernel.
#include "pll_runner.h"

namespace fmrx {

#ifdef FMRX_AB_PROF
__device__ unsigned long long g_cnt_prof[6];
#endif

namespace {

// The smallest float phase f with float(P + (double)f) >= c (phase_thr's T), always found: when
// phase_thr's window of four neighbours does not hold it (rare), a bisection over the ordered
// float line (32 halvings; "reaches" is monotone in f).
__device__ inline uint32_t fkey(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float fkey_inv(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ inline float phase_thr_exact(double P, uint32_t cb) {
    const float T = phase_thr(P, cb);
    if (T > -__builtin_inff()) return T;
    const float c = __builtin_bit_cast(float, cb);
    uint32_t lo = fkey(-__builtin_inff()), hi = fkey(__builtin_inff());  // reaches(lo) false, (hi) true
    for (int it = 0; it < 34 && hi - lo > 1u; it++) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (reaches(P, fkey_inv(mid), c)) hi = mid;
        else lo = mid;
    }
    return fkey_inv(hi);
}

template <int NI, int NC, int NW>
__global__ void __launch_bounds__(64 * (1 + NW)) __attribute__((amdgpu_waves_per_eu(1, 1)))
pll_cnt_kernel(const float* io, int n, int n_streams, size_t stride, double step, float norm_bw, float* st,
               float* out_base, size_t ostride, int inject, int miss, float lo, float hi, unsigned long long* stats,
               unsigned* redos) {
    constexpr int NP = NC + 2;  // row slots: T(c_base + l) l <= NC, +inf | NaN, e(c_base + l - 1), NaN
    constexpr int HC = NC / 2;  // candidates c0 - HC .. c0 + HC
    constexpr int RD = 4;       // intervals of step inputs in flight
    constexpr int EV = 64 * NW;                    // evaluator lanes
    constexpr int NE = (NI * NC + EV - 1) / EV;    // e items a lane an interval
    constexpr int NT = (NI * (NC + 1) + EV - 1) / EV;  // threshold items a lane an interval
    constexpr int CH = NI < 16 ? NI : 16;          // the chain's steps a burst of reads
    static_assert(NC % 2 == 1 && NP <= 64, "an odd window within a wave");
    static_assert(NI == 16 || NI == 32 || NI == 64 || NI == 128, "the counts in one or two VGPR rows");
    constexpr int NRW = NI > 64 ? 2 : 1;  // rows of counts: step J in lane J & 63 of row J >> 6
    // rings of four intervals (interval k in slot k & 3): the T and E rows of each pair of steps
    // interleaved by row slot (sR[.][p][l] = T_2p(l), E_2p(l), T_2p+1(l), E_2p+1(l): one 16-byte
    // read a lane gives the chain two steps' rows), bits(c_base) - 1 of each step (the trigArg
    // store), the chain's count of each step, its (integ, phase) at the interval's end, "redone
    // exactly"
    __shared__ float4 sR[4][NI / 2][NP];
    auto sT = [&](int sl, int J, int l) -> float& { return reinterpret_cast<float*>(&sR[sl][J >> 1][l])[2 * (J & 1)]; };
    auto sE = [&](int sl, int J, int l) -> float& { return reinterpret_cast<float*>(&sR[sl][J >> 1][l])[2 * (J & 1) + 1]; };
    __shared__ uint32_t sbase[4][NI];
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
    if (ni < 2 || !in_domain) {  // (counted in 16-step batches, as every runner counts)
        pll_stream_all_exact(f, w, t, in_domain, (unsigned long long)(n / kPllBatch), stats);
        return;
    }
    auto j0 = [](int k) { return NI * (k - 1); };  // interval k's first step (k >= 1)
    // the rows' constant slots, once: T slot NC + 1 = +inf (never counted), E slots 0 and NC + 1 NaN
    for (int q = threadIdx.x; q < 4 * NI; q += 64 * (1 + NW)) {
        sT(q / NI, q % NI, NC + 1) = __builtin_inff();
        sE(q / NI, q % NI, 0) = __builtin_nanf("");
        sE(q / NI, q % NI, NC + 1) = __builtin_nanf("");
    }

    if (w > 0) {
        const int el = (w - 1) * 64 + t;  // evaluator lane
        // item q of interval k: e item (J, kc) = (q / NC, q % NC), q = el + EV u (u < NE)
        auto ld = [&](int k, float (&v)[NE]) __attribute__((always_inline)) {
            const int kk = k <= ni ? k : ni;
#pragma unroll
            for (int u = 0; u < NE; u++) {
                const int q = min(el + EV * u, NI * NC - 1);
                v[u] = f.x[min(j0(kk) + q / NC + 1, n - 1)];  // the step the e is for
            }
        };
        auto put = [&](int k, float phase_ref, const float (&v)[NE]) __attribute__((always_inline)) {
            const int sl = k & 3;
#pragma unroll
            for (int u = 0; u < NE; u++) {
                const int q = el + EV * u;
                if (NE * EV > NI * NC && q >= NI * NC) break;
                const int J = q / NC, kc = q % NC;
                const double pr = f.pr_at(j0(k) + J);
                const uint32_t cb = __builtin_bit_cast(uint32_t, (float)(pr + (double)phase_ref));
                bool ok;
                const float e = pred_e_cert(__builtin_bit_cast(float, cb - (uint32_t)HC + (uint32_t)kc), v[u],
                                            pll_iv(v[u]), ok);
                // a window that is not of positive finite floats never certifies: c0 < 2^126
                const bool fin = cb > (uint32_t)HC && cb < 0x7F000000u;
                sE(sl, J, kc + 1) = ok && fin ? e : __builtin_nanf("");
            }
#pragma unroll
            for (int u = 0; u < NT; u++) {
                const int q = el + EV * u;
                if (NT * EV > NI * (NC + 1) && q >= NI * (NC + 1)) break;
                const int J = q / (NC + 1), kc = q % (NC + 1);
                const double pr = f.pr_at(j0(k) + J);
                const uint32_t cb = __builtin_bit_cast(uint32_t, (float)(pr + (double)phase_ref));
                sT(sl, J, kc) = phase_thr_exact(pr, cb - (uint32_t)HC + (uint32_t)kc);
                if (kc == 0) sbase[sl][J] = cb - (uint32_t)HC - 1u;
            }
        };
        // test hook pll_pipe_miss = -m (m >= 2): every interval from m - 1 on misses -- step 0's E row
        // NaN (the lanes of wave 1 that wrote it in put)
        auto hook_poison = [&](int k) {
            if (miss <= -2 && k >= -miss - 1 && w == 1 && t < NC) sE(k & 3, 0, t + 1) = __builtin_nanf("");
        };
        // wave 1: interval k's trigArgs, bits(c_base) - 1 + the chain's count (the chain stored a
        // redone interval itself)
        auto store = [&](int k) {
            if (w != 1) return;
            const int sl = k & 3;
            if (sexact[sl]) return;
#pragma unroll
            for (int r = 0; r < NRW; r++) {
                const int J = t + 64 * r;
                if (J < NI) f.out[j0(k) + J] = __builtin_bit_cast(float, sbase[sl][J] + (uint32_t)srow[sl][J]);
            }
        };
        float vq[RD][NE];
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
        PROF_ADD(t == 0 && w == 1, g_cnt_prof[2], ev_body);
        PROF_ADD(t == 0 && w == 1, g_cnt_prof[3], ev_wait);
        return;
    }

    // ---- the chain
    float integ = f.p.integ, phase = f.p.phase;
    // the carry: the E row of the previous trigArg and its count (SGPR); after an exact stretch
    // that trigArg's exact e in every lane
    float cE = pll_chain_begin(f, t, sst, sexact);
    uint32_t cC = 1;
    auto carry_exact = [&](float a, int k) {
        cE = exact_e(a, f.x[min(j0(k), n - 1)]);
        cC = 1;
    };
    int dem_i = 0;  // the interval the chain left after (pll_chain_leaves)
    unsigned long long n_redo = 0, n_inj = 0, ch_body = 0, ch_wait = 0;
    const int ls = t < NP ? t : NP - 1;  // this lane's row slot (lanes past the row read its last)
    // the last interval's verdict and pll_demote's history of them (SGPRs, pll_chain_leaves); the
    // start values are 0 but not constants to the compiler
    // (constants there made LLVM peel the first interval: a second copy of the chain loop)
    uint32_t prev_bad = n < 0 ? 1u : 0u, hist = n < 0 ? 1u : 0u;
    for (int i = 1; i <= ni && dem_i == 0; i++) {
        const unsigned long long p0 = PROF_T();
        const int is = i & 3;
        const float integ0 = integ, phase0 = phase;
        const bool leave = pll_chain_leaves<RD, NI, kPllDemoteMisses>(hist, prev_bad, i, ni, n, integ, phase);
        int row[NRW] = {};
        unroll_ic(
            [&](auto hc) {
                constexpr int H = decltype(hc)::value;
                // the burst's rows before its steps
                float T[CH], E[CH];
#pragma unroll
                for (int J = 0; J < CH; J += 2) {
                    const float4 r = sR[is][(H * CH + J) / 2][ls];
                    T[J] = r.x;
                    E[J] = r.y;
                    T[J + 1] = r.z;
                    E[J + 1] = r.w;
                }
                __builtin_amdgcn_sched_barrier(0);
                unroll_ic(
                    [&](auto jc) {
                        constexpr int J = decltype(jc)::value;
                        // step H CH + J: e of the previous trigArg (filter.cpp:161-162)
                        const float e = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cE), cC));
                        const float2v kv = float2v{f.Ki, f.Kp} * e;
                        integ = integ + kv.x;
                        phase = phase + (kv.y + integ);
                        // the count of thresholds the phase reaches: trigArg's place in the window + 1
                        cC = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(phase >= T[J]));
                        cE = E[J];
                        int rw = row[(H * CH + J) >> 6];
                        const uint32_t sc = cC;
                        asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(rw) : "s"(sc), "i"((H * CH + J) & 63));
                        row[(H * CH + J) >> 6] = rw;
                    },
                    std::make_integer_sequence<int, CH>{});
            },
            std::make_integer_sequence<int, NI / CH>{});
        // the interval's verdict: no NaN e taken (the phase) or carried (the last trigArg's), the
        // start state in pll_batch_fast's range; test hooks force misses
        const float ce = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cE), cC));
        // (one ballot: provably uniform, an SGPR -- the redo branch scalar, pll_demote's history SALU)
        const bool bad = __builtin_amdgcn_ballot_w64(!(phase == phase) || !(ce == ce) ||
                                                     !(fabsf(phase0) < kPllMaxPhase && fabsf(integ0) < kPllMaxInteg)) != 0 ||
                         i == min(miss, ni) || i == inj;
        if (bad) {  // uniform: redo the interval exactly from its start (the chain stores it)
            n_redo++;
            n_inj += i == inj ? 1 : 0;
            carry_exact(pll_redo_interval(f, i, NI, integ0, phase0, integ, phase), i + 1);
        }
#pragma unroll
        for (int r = 0; r < NRW; r++)
            if (t + 64 * r < NI) srow[is][t + 64 * r] = row[r];
        prev_bad = bad ? 1u : 0u;
        sst[is] = make_float4(integ, phase, __builtin_bit_cast(float, bad ? 1 : 0), __builtin_bit_cast(float, leave ? 1 : 0));
        sexact[is] = bad ? 1 : 0;
        const unsigned long long p1 = PROF_T();
        __syncthreads();
        ch_body += p1 - p0;
        ch_wait += PROF_T() - p1;
        if (leave) dem_i = i;  // (the evaluators leave after this interval's barrier too)
    }
    PROF_ADD(t == 0, g_cnt_prof[0], ch_body);
    PROF_ADD(t == 0, g_cnt_prof[1], ch_wait);
    PROF_ADD(t == 0, g_cnt_prof[4], (unsigned long long)ni);
    PROF_ADD(t == 0, g_cnt_prof[5], n_redo);
    // in 16-step batches, as every runner counts; "resumed": the inject hook's forced redos only;
    // fmrx_debug_pll_redos: by the range's trigOffset
    pll_chain_end(f, t, NI, dem_i ? dem_i : ni, dem_i != 0, integ, phase, n_inj * (NI / kPllBatch),
                  (unsigned long long)(n / kPllBatch), pll_redo_range(lo), n_redo, stats, redos);
}

}  // namespace

#ifdef FMRX_AB_PROF
static void print_cnt_prof() {
    unsigned long long h[6] = {};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_cnt_prof), sizeof h) == hipSuccess && h[4])
        std::fprintf(stderr, "pll_cnt prof: intervals %llu chain body %.1f wait %.1f, evaluator body %.1f wait %.1f "
                     "(shader cycles per interval), %llu redos\n", h[4], (double)h[0] / h[4], (double)h[1] / h[4],
                     (double)h[2] / h[4], (double)h[3] / h[4], h[5]);
}
#endif

#ifndef FMRX_CNT_NW
#define FMRX_CNT_NW 4  // evaluator waves of the [2^19, 2^21) count forms
#endif
#ifndef FMRX_CNT17_NW
#define FMRX_CNT17_NW 4  // evaluator waves of the [2^17, 2^19) count forms
#endif

// The count runner's forms (form: the trigOffset range as launch_pll numbers it), one stream a
// workgroup of 1 + NW waves (a CU), residency checked (pll_runner_launch).
int launch_pll_cnt(const PllRunnerArgs& a, int form) {
#ifdef FMRX_AB_PROF
    [[maybe_unused]] static const int prof_reg = std::atexit(print_cnt_prof);  // once
#endif
    if (a.n <= 0) return 0;
    constexpr auto ni = [](int f) { return pll_form(f, true).interval; };
    static_assert(ni(17) == FMRX_CNT17_NI && ni(18) == FMRX_CNT17_NI && ni(19) == FMRX_CNT19_NI &&
                      ni(20) == FMRX_CNT20_NI && ni(21) == FMRX_CNT21_NI,
                  "the instantiations below run pll_forms.h's intervals");
    const PllForm& f = pll_form(form, true);
    switch (form) {
        case 17:
        case 18:
            return pll_runner_launch<pll_cnt_kernel<FMRX_CNT17_NI, 31, FMRX_CNT17_NW>, 64 * (1 + FMRX_CNT17_NW)>(a, f);
        case 19:
            return pll_runner_launch<pll_cnt_kernel<FMRX_CNT19_NI, 15, FMRX_CNT_NW>, 64 * (1 + FMRX_CNT_NW)>(a, f);
        case 20:
            return pll_runner_launch<pll_cnt_kernel<FMRX_CNT20_NI, 15, FMRX_CNT_NW>, 64 * (1 + FMRX_CNT_NW)>(a, f);
        default:  // three waves a stream, as the three-wave runner it would replace
            return pll_runner_launch<pll_cnt_kernel<FMRX_CNT21_NI, 7, 2>, 64 * (1 + 2)>(a, f);
    }
}

}  // namespace fmrx
