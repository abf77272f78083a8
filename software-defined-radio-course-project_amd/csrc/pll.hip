// pll.hip — the PLL (src/filter.cpp:136-174) of the stereo pilot and the RDS carrier: the
// segment kernels (side data, the lane / many-stream speculative runners, the parallel check, the
// certified resume) and launch_pll, which runs the plan of pll_plan.cpp.  The other runners are
// translation units of their own (pll_sat.hip, pll_pred.hip, pll_pipe.hip, pll_idx.hip, pll_cnt.hip,
// pll_demote.hip: built without the SLP vectoriser; these kernels are faster with it, see the Makefile); the NCO pass that ends a
// call is stereo.hip's (launch_nco_pass), beside the audio kernel that inlines it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

#include "dsp_device.h"
#include "fmrx_internal.h"
#include "pll_cr.h"
#include "pll_device.h"
#include "pll_math.h"
#include "pll_plan.h"

namespace fmrx {

namespace {

// Side data of one PLL segment (pll_math.h pll_side): iv, pr for every sample, in
// parallel, from the trigOffset the segment starts with.  Two arrays of seg x n_streams
// doubles, sample pairs stream-minor: element (j, s) at (j/2 * n_streams + s) * 2 + j%2, so
// the PLL wave's lanes (one stream each) read consecutive 16-B pairs -- coalesced.

// One workgroup per tile of kPrepS streams x kPrepJ samples, transposed through LDS: rows of
// the stream-major input are read coalesced, the stream-minor pairs written coalesced.
constexpr int kPrepS = 16, kPrepJ = 64;
__global__ void __launch_bounds__(256) pll_prep_kernel(const float* io, int m, int n_streams, size_t stride,
                                                       double* side, size_t seg, const float* st, double step,
                                                       int* fail) {
    __shared__ double2 t_iv[kPrepJ / 2][kPrepS], t_pr[kPrepJ / 2][kPrepS], t_h[kPrepJ / 2][kPrepS];
    const int j0 = blockIdx.x * kPrepJ, s0 = blockIdx.y * kPrepS;
    // fail[] sentinel: 0 (= resume the whole segment exactly) until a runner claims the stream
    if (fail && blockIdx.x == 0 && threadIdx.x < kPrepS && s0 + (int)threadIdx.x < n_streams) fail[s0 + threadIdx.x] = 0;
    for (int e = threadIdx.x; e < kPrepS * kPrepJ; e += blockDim.x) {
        const int r = e / kPrepJ, c = e % kPrepJ, s = s0 + r, j = j0 + c;
        double iv = 0.0, pr = 0.0;
        if (s < n_streams && j < m) pll_side(io[(size_t)s * stride + j], st[8 * (size_t)s + 5], j, step, &iv, &pr);
        double* a = reinterpret_cast<double*>(&t_iv[c >> 1][r]);
        double* b = reinterpret_cast<double*>(&t_pr[c >> 1][r]);
        double* h = reinterpret_cast<double*>(&t_h[c >> 1][r]);
        a[c & 1] = iv;
        b[c & 1] = pr;
        h[c & 1] = iv < 0.0 ? 0.5 : 0.0;  // pll_batch_fast's half turn (SPEC)
    }
    __syncthreads();
    double2* siv = reinterpret_cast<double2*>(side);
    double2* spr = siv + seg * (size_t)n_streams / 2;
    double2* sh = spr + seg * (size_t)n_streams / 2;
    for (int e = threadIdx.x; e < kPrepS * kPrepJ / 2; e += blockDim.x) {
        const int jp = e / kPrepS, r = e % kPrepS, s = s0 + r;
        if (s < n_streams && j0 + 2 * jp < m) {
            const size_t a = (size_t)(j0 / 2 + jp) * n_streams + s;
            siv[a] = t_iv[jp][r];
            spr[a] = t_pr[jp][r];
            sh[a] = t_h[jp][r];
        }
    }
}

// The same side data stream-major (element (j, s) at s seg + j: each stream's samples
// contiguous; the half turns with zero gaps, 2 seg per stream), for the split kernels: a wave there works on at most 4 streams, so stream-minor
// rows would put every 16-B load of a wave on its own page (rows n_streams x 16 B apart).
// One thread per sample pair.
// with_h = 0: no half-turn plane (only pll_spec_lane_kernel reads it; the host passes 0 when that
// runner is not launched for the segment): 16 B a sample written instead of 32.
__global__ void __launch_bounds__(256) pll_prep_major_kernel(const float* io, int m, int n_streams, size_t stride,
                                                             double* side, size_t seg, const float* st, double step,
                                                             int with_h, int* fail) {
    const int s = blockIdx.y;
    const int jp = blockIdx.x * blockDim.x + threadIdx.x;
    // fail[] sentinel: 0 = pll_kernel resumes the whole segment on the certified path.  Every
    // runner that takes stream s overwrites it (fail[s] = nb, then the check's atomicMin), so a
    // stream no launched runner took -- a wrong trigOffset hint -- costs speed, never bits.
    if (fail && jp == 0) fail[s] = 0;
    if (2 * jp >= m) return;
    const float t0 = st[8 * (size_t)s + 5];
    double2 iv, pr, h;
    pll_side(io[(size_t)s * stride + 2 * jp], t0, 2 * jp, step, &iv.x, &pr.x);
    if (2 * jp + 1 < m) pll_side(io[(size_t)s * stride + 2 * jp + 1], t0, 2 * jp + 1, step, &iv.y, &pr.y);
    else iv.y = pr.y = 0.0;
    h.x = iv.x < 0.0 ? 0.5 : 0.0;
    h.y = iv.y < 0.0 ? 0.5 : 0.0;
    double2* siv = reinterpret_cast<double2*>(side);
    const size_t plane = seg * (size_t)n_streams / 2, a = (size_t)s * (seg / 2) + jp;
    siv[a] = iv;
    siv[plane + a] = pr;
    if (!with_h) return;
    // half turns in 32-B groups (h_2jp, h_2jp+1, 0, 0): pll_spec_lane_kernel's lane 2 reads the
    // first 16 B, the row's other lanes the zeros beside them (same cache line, no mask op)
    double2* sh = siv + 2 * plane + (size_t)s * seg + 2 * (size_t)jp;
    sh[0] = h;
    sh[1] = make_double2(0.0, 0.0);
}

// pll_math.h pll_state_at for the start of batch b (b NB steps into the segment), out of line.
__device__ __noinline__ PllPair pll_state_at_batch(float2 rec, float t0, int b, int nbatch, float a) {
    PllPair r;
    pll_state_at(r.p, r.ctx, rec.x, rec.y, t0, (long long)b * nbatch, a, DeviceLib{});
    return r;
}

// Streams per wave (spw, a power of two <= 64): lane t works on stream blockIdx.x spw + t % spw,
// and only lanes t < spw store.  The other lanes recompute their stream in lockstep (identical
// values): a wave with every lane active runs the serial chain ~15 % faster than one with a
// single live lane (one stream alone paid ~64 cycles a step of dependency stalls, a full wave
// none), and up to one wave per SIMD the streams run side by side at that single-wave speed.
//
// SPLIT (spw <= 4): streams by 16-lane row (lane t: stream blockIdx.x spw + (t / 16) % spw), so
// the batch's sin and cos can be one polynomial per lane, even lanes sin, odd lanes cos, shared
// by row broadcasts (pll_sincos_split); lane 0 of the stream's first row stores.
//
// The exact PLL (and, after pll_spec_kernel / pll_check_kernel, the fix-up): trigArg of step j
// goes to out[j] (out == io in place for the plain launch).  With `fail` (the first batch of
// each stream whose speculative result did not verify, nb when all did), the wave starts at
// the smallest such batch b0 of its streams, from the state recorded at the end of batch
// b0 - 1 -- exact for every stream of the wave, since none failed before b0 -- so a segment
// that verified costs only the tail.
template <int NB, bool SPLIT>
__global__ void __launch_bounds__(256) pll_kernel(float* io, int n, int n_streams, int spw, size_t stride,
                                                 const double* side, size_t seg, double step, float norm_bw,
                                                 float* st, float* out_base, size_t ostride, const int* fail,
                                                 const float2* rec, size_t rb, unsigned long long* stats) {
    const int t = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int s_lane = wave * spw + (SPLIT ? ((t >> 4) & (spw - 1)) : (t & (spw - 1)));
    const bool owner = (SPLIT ? ((t & 15) == 0 && (t >> 4) < spw) : t < spw) && s_lane < n_streams;
    const SplitCoef sc = split_coef((t & 1) != 0);
    const int s = s_lane < n_streams ? s_lane : n_streams - 1;
    float* x = io + (size_t)s * stride;
    float* out = out_base + (size_t)s * ostride;
    // pair q of batch b of this stream: element (b NB/2 + q) n_streams + s of a row of double2
    // (uniform base + lane offset: global loads with an SGPR base, no per-load address VALU)
    const double2* siv = reinterpret_cast<const double2*>(side);
    const double2* spr = siv + seg * (size_t)n_streams / 2;
    float* S = st + 8 * (size_t)s;
    const float Cp = static_cast<float>(2.666);
    const float Ci = static_cast<float>(3.555);
    const float Kp = norm_bw * Cp;
    const float Ki = (norm_bw * norm_bw) * Ci;
    PllState p{S[0], S[1], S[2], S[3], S[5]};
    PllCtx ctx{};
    ctx.valid = false;
    int i = 0;
    int b0 = 0;
    if (fail) {  // after the speculative runner: x is aligned (the host checked)
        int m = fail[s];
        if (stats && owner) {  // diagnostic counters (fmrx_debug_pll_stats), one atomic per stream
            const int nbs = n / NB;
            atomicAdd(stats, (unsigned long long)(nbs - m));
            atomicAdd(stats + 1, (unsigned long long)nbs);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
        b0 = m;
        if (b0 > 0) {
            const PllPair r = pll_state_at_batch(rec[(size_t)s * rb + b0 - 1], p.trig, b0, NB, out[b0 * NB - 1]);
            p = r.p;
            ctx = r.ctx;
        }
    }
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        // Batches of NB samples + side data (v, iv, pr: 20 B a sample) in ONE register set:
        // step j of batch b reloads the elements it has just consumed with batch b+1's (16-B
        // loads; see pll_batch_fast's refill), so every load has a whole batch to land and no
        // second set is needed (two sets overflow the 256 addressable VGPRs into AGPRs).
        float v[NB];
        double iv[NB], pr[NB];
        const int nb = n / NB;
        auto ld_v = [&](int b, int q) {  // floats 4q..4q+3
            *reinterpret_cast<float4*>(&v[4 * q]) = reinterpret_cast<const float4*>(x + b * NB)[q];
        };
        auto ld_d = [&](double (&dst)[NB], const double2* row, int b, int q) {  // doubles 2q, 2q+1
            *reinterpret_cast<double2*>(&dst[2 * q]) = SPLIT ? row[(size_t)s * (seg / 2) + b * (NB / 2) + q]
                                                        : (row + (size_t)(b * (NB / 2) + q) * n_streams)[s];
        };
        if (b0 < nb) {
#pragma unroll
            for (int q = 0; q < NB / 4; q++) ld_v(b0, q);
#pragma unroll
            for (int q = 0; q < NB / 2; q++) {
                ld_d(iv, siv, b0, q);
                ld_d(pr, spr, b0, q);
            }
        }
        for (int b = b0; b < nb; b++) {
            const int bn = b + 1 < nb ? b + 1 : b;  // the last batch reloads itself (no branch)
            // after step j: v[j], pr[j] are dead, and iv[j] (its sign was read at step j-1)
            auto refill = [&](int j) {
                if (j % 4 == 3) ld_v(bn, j / 4);
                if (j % 2 == 1) {
                    ld_d(iv, siv, bn, j / 2);
                    ld_d(pr, spr, bn, j / 2);
                }
            };
            // Optimistic batch: the 16 steps run straight-line on the certified fast paths
            // (pll_batch_fast: no per-step branch, no quadrant bookkeeping, no reciprocal);
            // only if some step of this stream could not be certified (~1e-4 per step) is the
            // batch redone from the saved state on the exact path with the library fallbacks,
            // from the inputs still in memory.  Bit-identical either way.
            const PllState p0 = p;
            const PllCtx ctx0 = ctx;
            float o[NB];
            float* xb = x + b * NB;
            float* ob = out + b * NB;
            if (pll_batch_fast<NB, SPLIT>(p, ctx, v, iv, pr, o, Ki, Kp, refill, sc)) {
                if (owner) {
#pragma unroll
                    for (int q = 0; q < NB / 4; q++)
                        reinterpret_cast<float4*>(ob)[q] = *reinterpret_cast<const float4*>(&o[4 * q]);
                }
            } else {  // rare: redo from the saved state on the exact path (duplicate rows of a
                      // wave write in lockstep, identical values; padding waves do not write)
                const PllPair r = pll_redo(p0, ctx0, xb, ob, NB, Ki, Kp, step, s_lane < n_streams);
                p = r.p;
                ctx = r.ctx;
            }
        }
        i = nb * NB;
    }
    if (i < n) {  // tail (and unaligned streams): exact steps
        const PllPair r = pll_redo(p, ctx, x + i, out + i, n - i, Ki, Kp, step, s_lane < n_streams);
        p = r.p;
    }
    if (owner) {
        S[0] = p.integ; S[1] = p.phase; S[2] = p.fbI; S[3] = p.fbQ; S[5] = p.trig;
    }
}

// ---- speculative PLL: runner + parallel exact check + fix-up ---------------------------------
//
// The certification inside pll_batch_fast is ~20 % of the serial step.  pll_spec_kernel runs
// the recurrence WITHOUT it (pll_batch_fast<SPEC>): trigArg to out, and (integ, phase) at the
// end of every batch to rec.  pll_check_kernel then recomputes every batch of every stream in
// parallel, one thread each, exactly (the certified batch, pll_step where it cannot certify)
// from the state the runner recorded at the end of the previous batch (batch 0: the true
// initial state st), and compares the 16 trigArgs and the end state bit for bit; fail[s] =
// the first batch that differs.  By
// induction every batch before fail[s] is exact.  pll_kernel (with `fail`) resumes from there
// on the certified path and runs the tail, so the result equals the plain launch bit for bit
// whatever the runner did; when everything verified it only runs the tail.
template <int NB>
__global__ void __launch_bounds__(256) pll_spec_kernel(const float* io, int n, int n_streams, int spw, size_t stride,
                                                      const double* side, size_t seg, double step, float norm_bw,
                                                      const float* st, float* out_base, size_t ostride, int* fail,
                                                      float2* rec, size_t rb, int inject) {
    const int t = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int s_lane = wave * spw + (t & (spw - 1));
    const bool owner = t < spw && s_lane < n_streams;
    const int s = s_lane < n_streams ? s_lane : n_streams - 1;
    const float* x = io + (size_t)s * stride;
    float* out = out_base + (size_t)s * ostride;
    const double2* siv = reinterpret_cast<const double2*>(side);
    const double2* spr = siv + seg * (size_t)n_streams / 2;
    const double2* sh = spr + seg * (size_t)n_streams / 2;
    const float* S = st + 8 * (size_t)s;
    const float Kp = norm_bw * static_cast<float>(2.666);
    const float Ki = (norm_bw * norm_bw) * static_cast<float>(3.555);
    PllState p{S[0], S[1], S[2], S[3], S[5]};
    const int nb = n / NB;
    if (owner) fail[s] = nb;
    // batch 0 on the exact path, as pll_kernel starts (a stream's first samples are often
    // exact zeros, where the uncertified rotation is NaN), which also sets the context
    PllCtx ctx{};
    ctx.valid = false;
    if (nb > 0) {
        const PllPair r = pll_redo(p, ctx, x, out, NB, Ki, Kp, step, s_lane < n_streams);
        p = r.p;
        ctx = r.ctx;
        if (owner) rec[(size_t)s * rb] = make_float2(p.integ, p.phase);
    }
    float v[NB];
    double iv[NB], pr[NB], hh[NB];
    auto ld_v = [&](int b, int q) {
        *reinterpret_cast<float4*>(&v[4 * q]) = reinterpret_cast<const float4*>(x + b * NB)[q];
    };
    auto ld_d = [&](double (&dst)[NB], const double2* row, int b, int q) {
        *reinterpret_cast<double2*>(&dst[2 * q]) = (row + (size_t)(b * (NB / 2) + q) * n_streams)[s];
    };
    if (nb > 1) {
#pragma unroll
        for (int q = 0; q < NB / 4; q++) ld_v(1, q);
#pragma unroll
        for (int q = 0; q < NB / 2; q++) {
            ld_d(iv, siv, 1, q);
            ld_d(pr, spr, 1, q);
            ld_d(hh, sh, 1, q);
        }
    }
    for (int b = 1; b < nb; b++) {
        const int bn = b + 1 < nb ? b + 1 : b;
        auto refill = [&](int j) {
            if (j % 4 == 3) ld_v(bn, j / 4);
            if (j % 2 == 1) {
                ld_d(iv, siv, bn, j / 2);
                ld_d(pr, spr, bn, j / 2);
                ld_d(hh, sh, bn, j / 2);
            }
            __builtin_amdgcn_sched_barrier(0);  // see pll_spec_lane_kernel
        };
        float o[NB];
        (void)pll_batch_fast<NB, false, true>(p, ctx, v, iv, pr, o, Ki, Kp, refill, SplitCoef{}, hh);
        if (inject >= 0 && b == 1 + (inject + s) % (nb - 1)) p.phase += 1.0e-3f;  // test hook: a wrong batch
        if (owner) {
            float* ob = out + b * NB;
#pragma unroll
            for (int q = 0; q < NB / 4; q++)
                reinterpret_cast<float4*>(ob)[q] = *reinterpret_cast<const float4*>(&o[4 * q]);
            rec[(size_t)s * rb + b] = make_float2(p.integ, p.phase);
        }
    }
}

// ---- the speculative runner with lane roles (split layout, 16-lane rows; spw <= 4) ------------
//
// pll_spec_kernel's recurrence with the lanes of a row (one stream) doing different work:
// sin and cos are one polynomial on even / odd lanes (pll_sincos_split), and lane 2 takes a
// third job.  The two reductions of a step's trigArg
// x -- r = x - nd pi/2 for sin/cos and the atan2 offset B = (m - h) 2 pi - x of the NEXT step
// (pll_offset_h) -- are the same five operations with different constants,
//     t = rint(fma(x, C1, H)) - H,   w = fma(-t, Clo, fma(-t, Chi, x)),
// (C1, Chi, Clo, H) = (2/pi, pi/2 hi, pi/2 lo, 0) on the sin/cos lanes (w = r, bit for bit:
// fma(x, C1, +0) is the rounded product) and (1/(2 pi), 2 pi hi, 2 pi lo, half turn) on lane 2
// of the row (w = -B, bit for bit: fma is odd under negating an operand pair), so lane 2
// computes the offset while the others compute r, and a third row broadcast hands -B to every
// lane.  The half turns reach lane 2 only: the other lanes load the zeros stored beside them.
// The batch state (fc, nfs, sn, cs, -B) stays in registers from batch to batch; nothing on
// the serial chain is a packed op but the first product (a packed f32 result read by the next
// instruction costs a wait state on gfx950).  ~36 VALU a step, 82 % of the wave's cycles issuing VALU
// (profiles/r02/runner/).  The result is checked by pll_check_kernel like pll_spec_kernel's.
template <int NB>
__global__ void __launch_bounds__(256) pll_spec_lane_kernel(const float* io, int n, int n_streams, int spw,
                                                           size_t stride, const double* side, size_t seg, double step,
                                                           float norm_bw, const float* st, float* out_base,
                                                           size_t ostride, int* fail, float2* rec, size_t rb,
                                                           int inject, int sat_ok, int pred_ok) {
    const int t = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int s_lane = wave * spw + ((t >> 4) & (spw - 1));
    const bool owner = (t & 15) == 0 && (t >> 4) < spw && s_lane < n_streams;
    const bool b_lane = (t & 15) == 2;
    const SplitCoef sc = split_coef((t & 1) != 0);
    const int s = s_lane < n_streams ? s_lane : n_streams - 1;
    const float* x = io + (size_t)s * stride;
    float* out = out_base + (size_t)s * ostride;
    const double2* siv = reinterpret_cast<const double2*>(side) + (size_t)s * (seg / 2);
    const double2* spr = reinterpret_cast<const double2*>(side) + seg * (size_t)n_streams / 2 + (size_t)s * (seg / 2);
    const float* S = st + 8 * (size_t)s;
    const float Kp = norm_bw * static_cast<float>(2.666);
    const float Ki = (norm_bw * norm_bw) * static_cast<float>(3.555);
    PllState p{S[0], S[1], S[2], S[3], S[5]};
    if (sat_ok && pll_sat_segment(spw, p.trig, step)) return;  // pll_sat_kernel's (pll_sat.hip)
    if (pred_ok && pll_pred_wave(p.trig, step)) return;        // pll_pred_kernel's (pll_pred.hip)
    const int nb = n / NB;
    if (owner) fail[s] = nb;
    PllCtx ctx{};
    ctx.valid = false;
    if (nb > 0) {  // batch 0 on the exact path (see pll_spec_kernel)
        const PllPair r = pll_redo(p, ctx, x, out, NB, Ki, Kp, step, s_lane < n_streams);
        p = r.p;
        ctx = r.ctx;
        if (owner) rec[(size_t)s * rb] = make_float2(p.integ, p.phase);
    }
    if (nb < 2) return;
    // reduction constants: 2 pi on the offset lane (lane 2), pi/2 on the sin/cos lanes
    const double C1 = b_lane ? kInv2Pi : kInvPio2;
    const double Chi = b_lane ? k2PiHi : kPio2Hi;
    const double Clo = b_lane ? k2PiLo : kPio2Lo;
    // half turns: lane 2 reads (h_j, h_j+1), the other lanes the zero pair beside it
    const double2* shl =
        reinterpret_cast<const double2*>(side) + seg * (size_t)n_streams + (size_t)s * seg + (b_lane ? 0 : 1);
    float v[NB];
    double iv[NB], pr[NB], hz[NB];
    auto ld_v = [&](int b, int q) {
        *reinterpret_cast<float4*>(&v[4 * q]) = reinterpret_cast<const float4*>(x + b * NB)[q];
    };
    auto ld_d = [&](double (&dst)[NB], const double2* row, int b, int q) {
        *reinterpret_cast<double2*>(&dst[2 * q]) = row[b * (NB / 2) + q];
    };
    auto ld_h = [&](int b, int q) {
        *reinterpret_cast<double2*>(&hz[2 * q]) = shl[2 * (b * (NB / 2) + q)];
    };
#pragma unroll
    for (int q = 0; q < NB / 4; q++) ld_v(1, q);
#pragma unroll
    for (int q = 0; q < NB / 2; q++) {
        ld_d(iv, siv, 1, q);
        ld_d(pr, spr, 1, q);
        ld_h(1, q);
    }
    // land batch 1 before the loop: the loop's back edge then carries the only loads in flight
    // at its top (a load issued last here would otherwise make every batch start with a full
    // wait, the waitcnt pass merging both edges)
    __builtin_amdgcn_s_waitcnt(0);
    // the state of batch 1's first step, as pll_batch_fast starts (every lane alike)
    const int q0 = ctx.q;
    const float u0 = (q0 & 1) ? p.fbQ : p.fbI, w0 = (q0 & 1) ? p.fbI : -p.fbQ;
    float fc = (q0 & 2) ? -u0 : u0, nfs = (q0 & 2) ? -w0 : w0;
    double sn = ctx.sn, cs = ctx.cs;
    double nB = -pll_offset_h(ctx.x, iv[0] < 0.0 ? 0.5 : 0.0);
    float integ = p.integ, phase = p.phase;
    // the rotation's Y = a sn + b cs of a sample from the current feedback (fc, nfs, sn, cs); the
    // one packed op on the chain: one instruction for both products, its wait state often filled
    // by scalar work (measured 0.4 % faster than two v_mul_f32)
    auto y_of = [&](float vv) -> double {
        const float2v ab = float2v{fc, nfs} * vv;
        return fma((double)ab.x, sn, (double)ab.y * cs);
    };
    for (int b = 1; b < nb; b++) {
        const int bn = b + 1 < nb ? b + 1 : b;
        float o[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const float e = (float)fma(y_of(v[j]), iv[j], -nB);
            const float ki_e = Ki * e;
            const float kp_e = Kp * e;
            integ = integ + ki_e;
            phase = phase + (kp_e + integ);
            const float arg = (float)(pr[j] + (double)phase);
            o[j] = arg;
            const double xa = (double)arg;
            const double H = hz[(j + 1) % NB];  // the next step's half turn on lane 2, else 0
            const double tq = rint(fma(xa, C1, H)) - H;
            const double w = fma(-tq, Clo, fma(-tq, Chi, xa));  // r, or -B on lane 2
            nB = row_bcast<2>(w);
            // sin/cos of r on the sin/cos lanes from the reduction's w
            const double W = split_w_horner(w * w, sc);
            sn = row_bcast<0>(w * W);
            cs = row_bcast<1>(W);
            fc = (float)cs;
            nfs = -(float)sn;
            // refill after step j: v[j], iv[j], pr[j] and hz[j] (read at step j - 1) are dead
            if (j % 4 == 3) ld_v(bn, j / 4);
            if (j % 2 == 1) {
                ld_d(iv, siv, bn, j / 2);
                ld_d(pr, spr, bn, j / 2);
                ld_h(bn, j / 2);
            }
            // keep each refill after the step that consumed its registers: hoisted loads
            // would overlap the old values and cost a register copy per element a batch
            __builtin_amdgcn_sched_barrier(0);
        }
        // test hook (a wrong batch), branch-free
        phase += (inject >= 0 && b == 1 + (inject + s) % (nb - 1)) ? 1.0e-3f : 0.0f;
        // every lane stores: the lanes of a row hold the same values, and rows past the last
        // stream recompute it bit for bit, so the writes agree; with no branch around them
        // the loads in flight across the loop's back edge need no full wait at its top
        float* ob = out + b * NB;
#pragma unroll
        for (int q = 0; q < NB / 4; q++)
            reinterpret_cast<float4*>(ob)[q] = *reinterpret_cast<const float4*>(&o[4 * q]);
        rec[(size_t)s * rb + b] = make_float2(integ, phase);
    }
}

// One thread per (batch, stream): NB exact steps from the recorded start, compared bit for
// bit.  The batch's side data (1/v, step x trigOffset) is recomputed, not read back: the kernel
// then reads only the input, the runner's trigArgs and records (125 vs 210 us a segment at
// 1,024 streams).
template <int NB>
__global__ void __launch_bounds__(64) pll_check_kernel(const float* io, int n, size_t stride, double step,
                                                       float norm_bw, const float* st, const float* out_base,
                                                       size_t ostride, int* fail, const float2* rec, size_t rb) {
    const int s = blockIdx.y;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int nb = n / NB;
    if (b >= nb) return;
    const float* S = st + 8 * (size_t)s;
    const float t0 = S[5];
    if (!pll_trig_domain(t0)) {  // pll_state_at's trigOffset needs it: the whole segment exactly
        if (b == 0) atomicMin(fail + s, 0);
        return;
    }
    const float* x = io + (size_t)s * stride + (size_t)b * NB;
    const float* o = out_base + (size_t)s * ostride + (size_t)b * NB;
    const float Kp = norm_bw * static_cast<float>(2.666);
    const float Ki = (norm_bw * norm_bw) * static_cast<float>(3.555);
    PllState p{S[0], S[1], S[2], S[3], t0};
    PllCtx ctx{};
    ctx.valid = false;
    const DeviceLib lib;
    if (b > 0) {  // inline: no call, no scratch frame for the returned state
        const float2 rb1 = rec[(size_t)s * rb + b - 1];
        pll_state_at(p, ctx, rb1.x, rb1.y, t0, (long long)b * NB, o[-1], lib);
    }
    bool same = true;
    bool done = false;
    // pr_j = step trig_j exactly as pll_side forms it (trig_j = min(t0 + j + 1, 2^24), integer-
    // valued t0 checked above), recomputed instead of read back: it rises with j, so the batch's
    // last value decides whether any is out of the fast path's range (pll_side's NaN)
    const double t0d = (double)t0;
    const double pr_last = step * fmin(t0d + (double)((long long)b * NB + NB), (double)kPllTrigStick);
    if (ctx.valid && fabs(pr_last) < kPllMaxPr) {  // the certified fast path (~2.5x cheaper than 16 pll_step)
        float v[NB], c[NB];
        double iv[NB], pr[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const size_t jj = (size_t)b * NB + j;
            v[j] = x[j];
            // 1/v recomputed too (reciprocal + one Newton step, ~2^-46 relative; pll_side's NaN
            // outside [kPllMinV, 1e300)): the batch's bound takes |Y/v| (|delta| + |eta|) with
            // |Y/v| <= 2^-23, so eta = 2^-46 adds ~2^-69 to kPllEBatch's 2e-14 (pll_math.h)
            const double vd = (double)v[j];
            const double r0 = __builtin_amdgcn_rcp(vd);
            const double r1 = fma(r0, fma(-vd, r0, 1.0), r0);
            iv[j] = (fabs(vd) >= (double)kPllMinV && fabs(vd) < 1.0e300) ? r1 : (double)NAN;
            pr[j] = step * fmin(t0d + (double)(jj + 1), (double)kPllTrigStick);
        }
        const PllState p0 = p;
        const PllCtx c0 = ctx;
        if (pll_batch_fast<NB, false>(p, ctx, v, iv, pr, c, Ki, Kp, [](int) {})) {
#pragma unroll
            for (int j = 0; j < NB; j++) same &= __float_as_uint(c[j]) == __float_as_uint(o[j]);
            done = true;
        } else {
            p = p0;
            ctx = c0;
        }
    }
    if (!done) {
        for (int j = 0; j < NB; j++) {
            const float a = pll_step(p, ctx, x[j], Ki, Kp, step, lib);
            same &= __float_as_uint(a) == __float_as_uint(o[j]);
        }
    }
    const float2 e = rec[(size_t)s * rb + b];
    same &= __float_as_uint(p.integ) == __float_as_uint(e.x) && __float_as_uint(p.phase) == __float_as_uint(e.y);
    if (!same) atomicMin(fail + s, b);
}

inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -2; }

// What the launches of one launch_pll call share.  out / ostride: where the steps' trigArgs go --
// the scratch's args (n a stream) behind the speculative runners, else io itself, in place.
struct PllCall {
    float* io;
    int n_streams;
    size_t stride;
    double step;
    float norm_bw;
    float* st;
    PllScratch sc;
    PllGeom g;
    float* out;
    size_t ostride;
    // test hooks (tests/test_gpu_parity.py): knob pll_inject = k, the runners corrupt batch
    // 1 + (k + s) % (nb - 1) of stream s (the self-certifying runners: a forced miss on one
    // interval), so the check and the fix-up from that batch (the exact redo) run on every stream;
    // pll_pipe_miss = k, the self-certifying runners report a miss on interval k of every launch
    int inject, pipe_miss;
    unsigned long long* stats;
    unsigned* redos;
    hipStream_t s;
};

// The launch of a Segment step that pll_step_stages files under `kind`.
void launch_segment_stage(const PllCall& c, const PllStep& p, int kind) {
    const PllGeom& g = c.g;
    const PllScratch& sc = c.sc;
    const dim3 grid((g.waves + g.wpg - 1) / g.wpg), block(64 * g.wpg);
    float* x = c.io + p.off;
    float* out = c.out + p.off;
    const int m = (int)p.len, ns = c.n_streams;
    const bool split = g.spw <= 4;  // the split kernels read stream-major side data
    int* fail = g.spec ? sc.fail : nullptr;
    switch (kind) {
        case kStPrep:
            if (split)
                hipLaunchKernelGGL(pll_prep_major_kernel, dim3(((m + 1) / 2 + 255) / 256, ns), dim3(256), 0, c.s, x, m,
                                   ns, c.stride, sc.side, g.seg, c.st, c.step, (g.spec && p.lane) ? 1 : 0, fail);
            else
                hipLaunchKernelGGL(pll_prep_kernel, dim3((m + kPrepJ - 1) / kPrepJ, (ns + kPrepS - 1) / kPrepS),
                                   dim3(256), 0, c.s, x, m, ns, c.stride, sc.side, g.seg, c.st, c.step, fail);
            break;
        case kStLane:
            if (split)  // it leaves waves only to the runners launched
                hipLaunchKernelGGL(pll_spec_lane_kernel<kPllBatch>, grid, block, 0, c.s, x, m, ns, g.spw, c.stride,
                                   sc.side, g.seg, c.step, c.norm_bw, c.st, out, c.ostride, sc.fail, sc.rec, g.rb,
                                   c.inject, p.sat ? 1 : 0, p.pred ? 1 : 0);
            else
                hipLaunchKernelGGL(pll_spec_kernel<kPllBatch>, grid, block, 0, c.s, x, m, ns, g.spw, c.stride, sc.side,
                                   g.seg, c.step, c.norm_bw, c.st, out, c.ostride, sc.fail, sc.rec, g.rb, c.inject);
            break;
        case kStSat:  // saturated streams (pll_sat_segment), which the lane kernel leaves to it
            launch_pll_sat(grid, block, c.s, x, m, ns, g.spw, c.stride, sc.side, g.seg, c.step, c.norm_bw, c.st, out,
                           c.ostride, sc.fail, sc.rec, g.rb, c.inject);
            break;
        case kStPred:  // waves from trigOffset 2^20 below the stick (pll_pred_wave)
            launch_pll_pred(g.waves, c.s, x, m, ns, g.spw, c.stride, sc.side, g.seg, c.step, c.norm_bw, c.st, out,
                            c.ostride, sc.fail, sc.rec, g.rb, c.inject, p.sat ? 1 : 0, 0);
            break;
        case kStCheck:
            hipLaunchKernelGGL(pll_check_kernel<kPllBatch>, dim3((m / kPllBatch + 63) / 64, ns), dim3(64), 0, c.s, x, m,
                               c.stride, c.step, c.norm_bw, c.st, out, c.ostride, sc.fail, sc.rec, g.rb);
            break;
        default:  // kStTail: resume at the first batch that did not verify, then the tail
            if (split)
                hipLaunchKernelGGL((pll_kernel<kPllBatch, true>), grid, block, 0, c.s, x, m, ns, g.spw, c.stride,
                                   sc.side, g.seg, c.step, c.norm_bw, c.st, out, c.ostride, fail, sc.rec, g.rb, c.stats);
            else
                hipLaunchKernelGGL((pll_kernel<kPllBatch, false>), grid, block, 0, c.s, x, m, ns, g.spw, c.stride,
                                   sc.side, g.seg, c.step, c.norm_bw, c.st, out, c.ostride, fail, sc.rec, g.rb, c.stats);
    }
}

// The arguments of a Range step's launches: the form's runner and the demoted kernel after it.
PllRunnerArgs runner_args(const PllCall& c, const PllStep& p) {
    return {c.s, c.io + p.off, (int)p.len, c.n_streams, c.stride, c.step, c.norm_bw, c.st, c.out + p.off, c.ostride,
            c.inject, c.pipe_miss, c.stats, c.redos};
}

int launch_demoted(const PllCall& c, const PllStep& p) { return launch_pll_demoted(runner_args(c, p)); }

// A Range step: the form's self-certifying launch on its runner, then (demote_after) the demoted
// kernel over the rest of the range of the streams that launch demoted.
int launch_range(const PllCall& c, const PllStep& p) {
    const PllRunnerArgs a = runner_args(c, p);
    int rc = 0;
    if (p.cnt)
        rc |= launch_pll_cnt(a, p.form);
    else if (p.form < 20)
        rc |= launch_pll_idx(a, p.form);
    else
        launch_pll_pipe(a, p.form);
    if (p.demote_after) rc |= launch_pll_demoted(a);
    return rc;
}

}  // namespace

PllScratch pll_scratch(double* side, int n, int n_streams) {
    const PllLayout l = pll_layout(n, n_streams);
    return {side, reinterpret_cast<float*>(side + l.args), reinterpret_cast<float2*>(side + l.rec),
            reinterpret_cast<int*>(side + l.fail), l.seg, l.rb};
}
size_t pll_side_doubles(int n, int n_streams) { return pll_layout(n, n_streams).doubles; }

// The PLL over n samples of n_streams streams, then the NCO of every sample in parallel
// (filter.cpp:136-174): the plan of the call (pll_plan: which runner runs which samples), each of
// its steps mapped to its launches (pll_step_stages names them, one stage record each), then the
// NCO.  FMRX_PLL_SPEC=0 (or rows not 16-byte aligned): the plain certified pll_kernel in place.
int launch_pll(float* io, int n, int n_streams, size_t stride, const PllLoop& loop, float* st, double* side,
               hipStream_t s, const PllHint& hint, unsigned long long* spec_stats, bool nco) {
    if (n <= 0) return 0;
    const PllKnobs& kn = hint.knobs;  // the context's switches (fmrx_debug_set_knob)
    const bool aligned = (reinterpret_cast<uintptr_t>(io) & 15) == 0 && stride % 4 == 0;
    const PllPlanIn in{n, n_streams, hint.n_simd, aligned, pll_loop_step(loop), hint.known, hint.trig_lo, hint.trig_hi,
                       kn, hint.demote_once};
    // the steps of the thread's last call are overwritten: no allocation once the capacity has
    // grown (the per-block seam calls this once a block)
    static thread_local std::vector<PllStep> steps;
    PllGeom g;
    pll_plan(in, &g, &steps);
    const PllScratch sc = pll_scratch(side, n, n_streams);
    const PllCall c{io, n_streams, stride, in.step, loop.norm_bw, st, sc, g, g.spec ? sc.args : io,
                    g.spec ? (size_t)n : stride, kn.inject, kn.pipe_miss, spec_stats, hint.redos, s};
    StageTimer* tm = hint.timer;
    auto timed = [&](int kind, double nsteps, auto&& launch) {
        const int t = tm ? tm->begin(s) : -1;
        launch();
        if (tm) tm->end(t, kind, nsteps, s);
    };
    int rc = 0;
    for (const PllStep& p : steps)
        pll_step_stages(p, g, [&](int kind, double nsteps) {
            timed(kind, nsteps, [&] {
                if (p.op == PllStep::Segment) launch_segment_stage(c, p, kind);
                else rc |= p.op == PllStep::Range ? launch_range(c, p) : launch_demoted(c, p);
            });
        });
    // the NCO of every sample from its trigArg (filter.cpp:170), in parallel, over the input in place
    if (nco)
        timed(kStNco, 0.0, [&] {
            launch_nco_pass(io, n, n_streams, stride, c.out, c.ostride, loop, st, s);
        });
    else if (!g.spec)  // the trigArgs are in io itself: launch_pll_nco reads them from `side`
        (void)hipMemcpy2DAsync(sc.args, (size_t)n * sizeof(float), io, stride * sizeof(float),
                               (size_t)n * sizeof(float), n_streams, hipMemcpyDeviceToDevice, s);
    return rc ? -2 : ok();
}

int launch_pll_nco(float* io, int n, int n_streams, size_t stride, const PllLoop& loop, float* st, double* side,
                   hipStream_t s) {
    if (n <= 0) return 0;
#ifdef FMRX_AB_NO_NCO
    return 0;  // A/B build only (timing: what the NCO beside the chains costs them; output wrong)
#endif
    launch_nco_pass(io, n, n_streams, stride, pll_scratch(side, n, n_streams).args, (size_t)n, loop, st, s);
    return ok();
}

}  // namespace fmrx
