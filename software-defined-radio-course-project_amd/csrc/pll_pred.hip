// pll_pred.hip — the speculative PLL runner with predicted trigArgs (src/filter.cpp:157-171) for
// segments from trigOffset 2^20 on, the 2^24 stick included; streams by 16-lane row (spw <= 4),
// like pll_spec_lane_kernel.
//
// trigArg_j = float(P_j + phase_j) with P_j = 2 pi (f/Fs) trigOffset_j in double (pll_side's pr).
// From 2^20 steps on, P_j's float grid is 2^-5 rad or coarser (2^-2 from 2^22, 1 once trigOffset
// has stuck) while the phase moves by |Kp e + integ| < 0.05 rad a step and stays within a few
// radians: a candidate formed ahead of the chain from an EARLIER phase, c0 = float(P_j +
// phase_ref), is within one float of the true trigArg on 99 % of the steps below 2^22 and on
// every step of the bench stream from there on (tools/pll_predict.cpp, phase_ref from two batches
// back).  So the feedback of a step -- sin, cos and the atan2 offset of trigArg_j,
// which the NEXT step's error e needs -- need not wait for the serial chain.
//
// Two waves per workgroup (one group of spw streams; the two land on different SIMDs of the CU,
// tools/ubench_wgsimd.hip, profiles/r03/ubench_wgsimd.txt):
//   wave 1 (the evaluator) computes, for every step l of batch b + 1, the next step's error e for
//     the three candidates c0 - 1, c0, c0 + 1 ulp (lane l of a row; phase_ref = the phase at the
//     start of batch b; with one stream the four rows split the three candidates and the rest),
//     and stores them, the thresholds float(S) >= c of two candidates as doubles (thr_of) and P_l
//     in LDS;
//   wave 0 (the chain) runs batch b from LDS: per step the candidate of trigArg_{j-1}, chosen by
//     comparing the double sum S_{j-1} = P + phase (before its rounding to float) with the two
//     thresholds, (Ki e, Kp e), integ += Ki e, phase += Kp e + integ, S_j = P_j + phase; trigArg
//     = float(S_j) off the chain.
// One barrier per batch; the chain's wave issues nothing else, so its step is the dependency
// chain itself.  A step whose trigArg is not a candidate sets the batch's miss flag: the chain
// redoes the batch from its start, evaluating such steps' e directly (uniform loads of the step's
// input, sin and cos in every lane).  The arithmetic of e is pll_spec_lane_kernel's (e =
// float(fma(Y, 1/v, B)), the same sin/cos polynomials and offsets), and the output -- trigArgs and
// the per-batch (integ, phase) records -- is checked by pll_check_kernel like every runner's, so
// the result is the certified path's bit for bit whatever was predicted.
// (The self-certifying runners that took over most of its ranges are pll_pipe.hip, pll_idx.hip and
// pll_cnt.hip; pll_runner.h holds what they share with this one.)
#include "pll_runner.h"

namespace fmrx {

#ifdef FMRX_AB_PROF
__device__ unsigned long long g_pred_prof[6];
#endif

namespace {

template <int NB>
__global__ void __launch_bounds__(128) pll_pred_kernel(const float* io, int n, int n_streams, int spw, size_t stride,
                                                      const double* side, size_t seg, double step, float norm_bw,
                                                      const float* st, float* out_base, size_t ostride, int* fail,
                                                      float2* rec, size_t rb, int inject, int sat_ok,
                                                      int pipe_on) {
    // per step of the batch, double-buffered by batch parity: the phase thresholds of c0 and
    // c0 + 1 ulp, the bits of c0 - 1 ulp and the next step's e for c0 - 1 ulp (sa); its e for c0
    // and c0 + 1 ulp and P (sb: e_0, e_p, P as two words).  Two 16-B reads a step: the chain
    // loads a whole batch into registers before its first step.
    __shared__ float4 sa[2][4][NB];
    __shared__ float4 sb[2][4][NB];
    __shared__ float ph[2][4];  // the phase at the start of batch k, slot k & 1
    const int t = threadIdx.x & 63;
    const bool chain = threadIdx.x < 64;
    const int q = (t >> 4) & (spw - 1);  // the row's stream in the group
    const int s_lane = blockIdx.x * spw + q;
    const bool owner = chain && (t & 15) == 0 && (t >> 4) < spw && s_lane < n_streams;
    const int s = s_lane < n_streams ? s_lane : n_streams - 1;
    const int l = t & 15;
    const float* x = io + (size_t)s * stride;
    float* out = out_base + (size_t)s * ostride;
    const float* S = st + 8 * (size_t)s;
    const float Kp = norm_bw * static_cast<float>(2.666);
    const float Ki = (norm_bw * norm_bw) * static_cast<float>(3.555);
    PllState p{S[0], S[1], S[2], S[3], S[5]};
    // both waves alike: the lane runner's waves, or the saturated runner's when it is launched
    if (!pll_pred_wave(p.trig, step) || (sat_ok && pll_sat_segment(spw, p.trig, step)) ||
        (pipe_on && pll_pipe_stream(p.trig, step)))
        return;
    const int nb = n / NB;
    if (nb < 2) {  // batch 0 alone, exactly (no barrier is reached)
        if (chain) {
            if (owner) fail[s] = nb;
            if (nb > 0) {
                PllCtx ctx{};
                ctx.valid = false;
                const PllPair r = pll_redo(p, ctx, x, out, NB, Ki, Kp, step, s_lane < n_streams);
                if (owner) rec[(size_t)s * rb] = make_float2(r.p.integ, r.p.phase);
            }
        }
        return;
    }
    // side data, stream-major (pll_prep_major_kernel): 1/v and pr planes
    const double* ivs = side + (size_t)s * seg;
    const double* prs = side + seg * (size_t)n_streams + (size_t)s * seg;

    if (!chain) {
        // ---- the evaluator: batch b + 1's candidates during the chain's batch b
        // this lane's data for batch b: pr of step l, the input of step l + 1 (the step its e is
        // for; the segment's last sample stands in past the end)
        auto ld = [&](int b, float& v, double& iv, double& pr) {
            const int jn = min(b * NB + l + 1, n - 1);
            v = x[jn];
            iv = ivs[jn];
            pr = prs[b * NB + l];
        };
        auto put = [&](int b, float phase_ref, float v, double iv, double pr) {
            const float c0 = (float)(pr + (double)phase_ref);
            const uint32_t cb = __builtin_bit_cast(uint32_t, c0);
            const uint2 prw = __builtin_bit_cast(uint2, pr);
            if (spw == 1) {
                // one stream: its four rows share the work -- rows 0-2 the e of candidates
                // c0 - 1, c0, c0 + 1 ulp, row 3 the thresholds, the miss bits and P
                const int r = t >> 4;
                float* a = reinterpret_cast<float*>(&sa[b & 1][0][l]);
                float* bb = reinterpret_cast<float*>(&sb[b & 1][0][l]);
                if (r < 3) {
                    const float e = pred_e(__builtin_bit_cast(float, cb + (uint32_t)(r - 1)), v, iv);
                    if (r == 0) a[3] = e;
                    else bb[r - 1] = e;
                } else {
                    const float T0 = phase_thr(pr, cb), T1 = phase_thr(pr, cb + 1u);
                    // a candidate that is not a positive finite float or a threshold outside its
                    // window: every trigArg misses the step's candidates
                    const bool ok = c0 > 0.0f && c0 < 3.0e38f && T0 > -__builtin_inff() && T1 > -__builtin_inff();
                    a[0] = T0;
                    a[1] = T1;
                    a[2] = __builtin_bit_cast(float, ok ? cb - 1u : 0xFFFFFFFFu);
                    bb[2] = __builtin_bit_cast(float, prw.x);
                    bb[3] = __builtin_bit_cast(float, prw.y);
                }
                return;
            }
            const float em = pred_e(__builtin_bit_cast(float, cb - 1u), v, iv);
            const float e0 = pred_e(c0, v, iv);
            const float ep = pred_e(__builtin_bit_cast(float, cb + 1u), v, iv);
            const float T0 = phase_thr(pr, cb), T1 = phase_thr(pr, cb + 1u);
            const bool ok = c0 > 0.0f && c0 < 3.0e38f && T0 > -__builtin_inff() && T1 > -__builtin_inff();
            if ((t >> 4) < spw) {
                sa[b & 1][q][l] = make_float4(T0, T1, __builtin_bit_cast(float, ok ? cb - 1u : 0xFFFFFFFFu), em);
                sb[b & 1][q][l] = make_float4(e0, ep, __builtin_bit_cast(float, prw.x), __builtin_bit_cast(float, prw.y));
            }
        };
        // ring of 4 batches of step data: batch k in slot k & 3, refilled right after its use,
        // so each load has ~3 batches to land
        float vq[4];
        double ivq[4], prq[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int k = 1 + u;  // batches 1..4 in slots 1, 2, 3, 0
            ld(k < nb ? k : nb - 1, vq[k & 3], ivq[k & 3], prq[k & 3]);
        }
        // batch 1 from the phase at the start of batch 0: the initial state
        put(1, p.phase, vq[1], ivq[1], prq[1]);
        ld(5 < nb ? 5 : nb - 1, vq[1], ivq[1], prq[1]);
        __syncthreads();  // (prologue)
        unsigned long long ev_body = 0, ev_wait = 0;
        // iteration b: batch b + 1's candidates from the phase at the start of batch b; groups
        // of four iterations from b0 = 1 (mod 4), so the ring slots are compile-time
        for (int b0 = 1; b0 < nb; b0 += 4) {
            unroll_ic(
                [&](auto uc) {
                    constexpr int u = decltype(uc)::value;
                    constexpr int sl = (2 + u) & 3;  // slot of batch b + 1 = (b0 + u + 1) & 3
                    const int b = b0 + u;
                    if (b < nb) {
                        const unsigned long long p0 = PROF_T();
                        if (b + 1 < nb) {
                            put(b + 1, ph[b & 1][q], vq[sl], ivq[sl], prq[sl]);
                            const int bq = b + 5 < nb ? b + 5 : nb - 1;
                            ld(bq, vq[sl], ivq[sl], prq[sl]);
                        }
                        const unsigned long long p1 = PROF_T();
                        __syncthreads();
                        ev_body += p1 - p0;
                        ev_wait += PROF_T() - p1;
                    }
                },
                std::make_integer_sequence<int, 4>{});
        }
        PROF_ADD(t == 0, g_pred_prof[2], ev_body);
        PROF_ADD(t == 0, g_pred_prof[3], ev_wait);
        return;
    }

    // ---- the chain
    if (owner) fail[s] = nb;
    PllCtx ctx{};
    ctx.valid = false;
    {  // batch 0 on the exact path (see pll_spec_kernel)
        const PllPair r = pll_redo(p, ctx, x, out, NB, Ki, Kp, step, s_lane < n_streams);
        p = r.p;
        ctx = r.ctx;
        if (owner) rec[(size_t)s * rb] = make_float2(p.integ, p.phase);
    }
    float integ = p.integ, phase = p.phase;
    float tlast = (float)ctx.x;  // the last trigArg done
    // the carry: the candidates of the previous batch's last trigArg -- after the exact batch 0
    // its e directly (all three slots alike, so the thresholds do not matter)
    float4 carry_a, carry_b;
    {
        const float e = pred_e(tlast, x[NB], ivs[NB]);
        carry_a = make_float4(0.0f, 0.0f, __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, tlast) - 1u), e);
        carry_b = make_float4(e, e, 0.0f, 0.0f);
    }
    if (l == 0) ph[1][q] = phase;  // the start of batch 1, for the evaluator's batch 2
    __syncthreads();               // (prologue)
    unsigned long long ch_body = 0, ch_wait = 0;
    for (int b = 1; b < nb; b++) {
        const unsigned long long p0 = PROF_T();
        const int bp = b & 1;
        const float integ0 = integ, phase0 = phase, tlast0 = tlast;
        // the whole batch's data into registers first (32 reads), so no step waits on LDS
        float4 A[NB], Bv[NB];
#pragma unroll
        for (int J = 0; J < NB; J++) {
            A[J] = sa[bp][q][J];
            Bv[J] = sb[bp][q][J];
        }
        __builtin_amdgcn_sched_barrier(0);
        auto P_of = [&](int J) {
            return __builtin_bit_cast(double, make_uint2(__builtin_bit_cast(uint32_t, Bv[J].z),
                                                         __builtin_bit_cast(uint32_t, Bv[J].w)));
        };
        // step J's selection data: those of trigArg_{J-1} (the carry for J = 0)
        auto sel_of = [&](auto jc, float4& a, float4& bb) {
            constexpr int J = decltype(jc)::value;
            if constexpr (J == 0) {
                a = carry_a;
                bb = carry_b;
            } else {
                a = A[J - 1];
                bb = Bv[J - 1];
            }
        };
        float o[NB];
        // max over the steps of bits(trigArg) - bits(c0 - 1 ulp): > 2 is a miss.  It starts with
        // the previous batch's last trigArg against the carry: a miss there (also left by that
        // batch's redo, which does not reach the step after it) is this batch's step 0
        uint32_t dmax = __builtin_bit_cast(uint32_t, tlast) - __builtin_bit_cast(uint32_t, carry_a.z);
        unroll_ic(
            [&](auto jc) {
                constexpr int J = decltype(jc)::value;
                float4 a, bb;
                sel_of(jc, a, bb);
                // the chain: two compares of the phase, e, (Ki e, Kp e), the three float updates
                const float e = pick(phase, make_float4(a.x, a.y, a.w, bb.x), bb.y);
                const float2v k = float2v{Ki, Kp} * e;
                integ = integ + k.x;
                phase = phase + (k.y + integ);
                // off the chain: trigArg (filter.cpp:165) and its candidate check
                const float arg = (float)(P_of(J) + (double)phase);
                o[J] = arg;
                dmax = max(dmax, __builtin_bit_cast(uint32_t, arg) - __builtin_bit_cast(uint32_t, A[J].z));
            },
            std::make_integer_sequence<int, NB>{});
        tlast = o[NB - 1];
        if (__builtin_expect(dmax > 2u, 0)) {
            // a trigArg outside its candidates: redo the batch, evaluating the e of a step that
            // follows a miss directly (rows without a miss are masked off here)
            integ = integ0;
            phase = phase0;
            float tprev = tlast0;
            const int j0 = b * NB;
            unroll_ic(
                [&](auto jc) {
                    constexpr int J = decltype(jc)::value;
                    float4 a, bb;
                    sel_of(jc, a, bb);
                    float e = pick(phase, make_float4(a.x, a.y, a.w, bb.x), bb.y);
                    if (__builtin_bit_cast(uint32_t, tprev) - __builtin_bit_cast(uint32_t, a.z) > 2u)
                        e = pred_e(tprev, x[j0 + J], ivs[j0 + J]);
                    const float2v k = float2v{Ki, Kp} * e;
                    integ = integ + k.x;
                    phase = phase + (k.y + integ);
                    tprev = (float)(P_of(J) + (double)phase);
                    o[J] = tprev;
                },
                std::make_integer_sequence<int, NB>{});
            tlast = o[NB - 1];
        }
        if (inject >= 0 && b == 1 + (inject + s) % (nb - 1)) {  // test hook: a wrong batch
            phase += 1.0e-3f;
            tlast = (float)(P_of(NB - 1) + (double)phase);
        }
        // every lane stores: the rows of a stream hold the same values, and rows past the last
        // stream recompute it bit for bit (their evaluator rows too), so the writes agree
        float* ob = out + b * NB;
#pragma unroll
        for (int qq = 0; qq < NB / 4; qq++)
            reinterpret_cast<float4*>(ob)[qq] = *reinterpret_cast<const float4*>(&o[4 * qq]);
        rec[(size_t)s * rb + b] = make_float2(integ, phase);
        carry_a = A[NB - 1];  // the candidates of step 15: step 0 of batch b + 1
        carry_b = Bv[NB - 1];
        if (l == 0) ph[(b + 1) & 1][q] = phase;
        const unsigned long long p1 = PROF_T();
        __syncthreads();
        ch_body += p1 - p0;
        ch_wait += PROF_T() - p1;
    }
    PROF_ADD(t == 0, g_pred_prof[0], ch_body);
    PROF_ADD(t == 0, g_pred_prof[1], ch_wait);
    PROF_ADD(t == 0, g_pred_prof[4], (unsigned long long)(nb - 1));
}
}  // namespace

#ifdef FMRX_AB_PROF
static void print_pred_prof() {
    unsigned long long h[6] = {};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_pred_prof), sizeof h) == hipSuccess && h[4])
        std::fprintf(stderr, "pll_pred prof: batches %llu chain body %.1f wait %.1f, evaluator body %.1f wait %.1f "
                     "(shader cycles per batch)\n", h[4], (double)h[0] / h[4], (double)h[1] / h[4],
                     (double)h[2] / h[4], (double)h[3] / h[4]);
}
#endif

void launch_pll_pred(int waves, hipStream_t s, const float* io, int n, int n_streams, int spw, size_t stride,
                     const double* side, size_t seg, double step, float norm_bw, const float* st, float* out,
                     size_t ostride, int* fail, float2* rec, size_t rb, int inject, int sat_ok, int pipe_on) {
#ifdef FMRX_AB_PROF
    [[maybe_unused]] static const int prof_reg = std::atexit(print_pred_prof);  // once
#endif
    hipLaunchKernelGGL(pll_pred_kernel<kPllBatch>, dim3(waves), dim3(128), 0, s, io, n, n_streams, spw, stride, side,
                       seg, step, norm_bw, st, out, ostride, fail, rec, rb, inject, sat_ok, pipe_on);
}

}  // namespace fmrx
