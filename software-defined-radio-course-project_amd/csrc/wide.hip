// wide.hip — the decimating down-converter in front of the tuner: a capture at cap_fs = D rf_fs
// (D = 2..10) -> per station: coarse rotation at the capture rate -> low-pass -> decimate by D ->
// cf32 rows at rf_fs, which tuner.hip then reads as an FMRX_IQ_F32 stream tuned to the fine part of
// the offset.  Every station reads the ONE capture.
//
// Arithmetic (the contract the tests check bit for bit).  An offset f splits into
// f_c = q rf_fs / 4 and f_r = f - f_c (rate_split at up = 1, wide_design.cpp).  With N = 4 D / gcd(|q|, 4 D),
// k = (q / gcd) mod N, the table c[p] = (float)cos(2 pi p / N), s[p] = (float)sin(2 pi p / N) and
// p = (k n) mod N, wide pair n (absolute index) with the format's normalised samples x_i, x_q becomes
//   I' = fl(fl(x_i c[p]) + fl(x_q s[p])),  Q' = fl(fl(x_q c[p]) - fl(x_i s[p]))
// and with h = the 16 D + 1 tap low-pass (cut-off 3 rf_fs / 8 at cap_fs)
//   y_i[m] = sum_k h[k] I'[D m - k],  acc = fl(acc + fl(h[k] x)) from 0 in ascending k,
// y_q alike from Q'; pairs in front of the stream are 0.  The integer formats are normalised first
// (one exact multiply by a power of two a sample), so every operation is the definition's.
//
// Decomposition.  A workgroup (one wave) walks a run of chunks of 256 outputs of one station.  Per
// chunk: coalesced unit loads (two pairs a lane, prefetched one chunk ahead), raw -> float, rotation
// against the station's table (LDS, at most 40 entries), rotated pairs to LDS in D polyphase rows:
// pair b of the buffer (16 D history pairs, then the chunk's) sits at [b mod D][b div D].  Lanes own
// consecutive outputs m, so tap k = D j + i reads row (-i) mod D at column 16 + m - j - (i > 0):
// consecutive lanes read consecutive addresses for every tap.  The taps are wave-uniform loads.  The
// last 16 D pairs of a chunk are the next chunk's history; the first chunk of a workgroup rebuilds
// its history from the raw pairs in front of it (the capture, or the context's history of the
// previous call), and a phase is a function of the absolute index alone, so there is no carried state.
#include <hip/hip_runtime.h>

#include "dsp_device.h"
#include "iq_fmt.h"
#include "tuner.h"
#include "wide.h"

namespace fmrx {

namespace {

constexpr int kNT = 64;  // one wave a workgroup
constexpr int kR = 4;    // outputs a lane and chunk
constexpr int kG = 4;    // taps a group of the FIR loop

template <int D>
struct WideCfg {
    static constexpr int CM = kNT * kR;       // outputs per chunk
    static constexpr int P = CM * D;          // wide pairs per chunk
    static constexpr int H = 16 * D;          // history pairs (taps - 1)
    static constexpr int T = 16 * D + 1;      // taps
    static constexpr int W = 16 + CM + 1;     // columns of a polyphase row (one pad)
    static constexpr int NLD = (P / 2) / kNT; // unit (2-pair) loads per lane and chunk
    static constexpr int NGRP = (T + kG - 1) / kG;  // tap groups
    static_assert((P / 2) % kNT == 0, "whole loads per chunk");
    static_assert(CM == kWideChunk, "wide_segments counts chunks of kWideChunk outputs");
};

// The two pairs of unit w, normalised and rotated by table entries a and b, to buffer pairs b0, b0 + 1
template <int D, int F>
__device__ inline void stage_unit(float2* xb, int b0, typename IqFmt<F>::Raw w, float2 a, float2 b) {
    const float4 r = rotate_scaled<F>(w, a, b);
    constexpr int W = WideCfg<D>::W;
    const int b1 = b0 + 1;
    xb[(b0 % D) * W + b0 / D] = make_float2(r.x, r.y);
    xb[(b1 % D) * W + b1 / D] = make_float2(r.z, r.w);
}

template <int D, int F>
__global__ void __launch_bounds__(kNT) wide_ddc_kernel(DdcLaunch L, const float* __restrict__ h) {
    using C = WideCfg<D>;
    using Fmt = IqFmt<F>;
    using Raw = typename Fmt::Raw;
    constexpr int PB = Fmt::PB;
    constexpr int NT = kNT, R = kR, CM = C::CM, P = C::P, H = C::H, W = C::W, NLD = C::NLD;
    __shared__ float2 rot[kWideMaxN];  // the station's table: (c[p], s[p]), p < N
    __shared__ float2 xb[D * W];       // rotated (I', Q') pairs, D polyphase rows

    const int tid = threadIdx.x;
    const long long n_out = L.n_out;
    // chunk indices fit 32 bits for any HBM-resident capture; positions stay 64-bit
    const int n_chunks = (int)((n_out + CM - 1) / CM);
    const int stream = (int)blockIdx.x / L.segs;
    const int seg = (int)blockIdx.x - stream * L.segs;
    const int c0 = (int)((long long)seg * n_chunks / L.segs);
    const int c1 = (int)((long long)(seg + 1) * n_chunks / L.segs);
    if (c0 >= c1) return;
    const int c_full = (int)(L.stream_bytes / (PB * P));  // chunks lying wholly in the data

    const uint8_t* in = L.iq;
    const uint8_t* hist = L.hist;
    const long long total = (long long)L.stream_bytes;
    constexpr long long hb = (long long)H * PB;

    // ---- the station's rotator: table to LDS, phases of this workgroup's first pairs
    const WideStream ws = L.streams[stream];
    const uint32_t N = ws.N, k = ws.k;  // N <= kWideMaxN < NT
    if ((uint32_t)tid < N) rot[tid] = L.tables[(size_t)stream * kRateMaxN + tid];
    const RotatorPhase rp(N, k, L.first_pair, (uint32_t)tid, (uint32_t)NT, (uint32_t)P);
    uint32_t pc = rp.of((long long)c0 * P);  // phase of chunk c's first pair
    wave_sync();  // table staged

    // ---- prologue: the history in front of chunk c0 (pairs [c0 P - H, c0 P)) to buffer pairs [0, H)
    for (int i = tid; i < H / 2; i += NT) {
        const long long rel = (long long)c0 * P - H + 2 * i;
        const Raw w = load_unit<F>(in, hist, rel * PB, total, hb);
        const uint32_t p0 = rp.of(rel);
        stage_unit<D, F>(xb, 2 * i, w, rot[p0], rot[addmod(p0, k, N)]);
    }
    // Input prefetch, one chunk ahead: always the same coalesced unit loads, from a base clamped
    // into the capture so that they never leave it; a chunk that runs past the end (c >= c_full) is
    // rebuilt at staging time.
    Raw pf[NLD];
    auto fetch = [&](int cc) {
        if (c_full == 0) return;  // capture shorter than a chunk: every chunk is rebuilt
        const int cl = cc < c_full ? cc : c_full - 1;
        const Raw* src = reinterpret_cast<const Raw*>(in + (size_t)cl * (PB * P)) + tid;
#pragma unroll
        for (int l = 0; l < NLD; l++) pf[l] = src[l * NT];
    };
    fetch(c0);

    float2* yrow = reinterpret_cast<float2*>(L.y + (size_t)stream * L.y_stride);
    for (int c = c0; c < c1; c++) {
        // ---- stage chunk c: lane u rotates pairs 2u, 2u + 1
        if (c >= c_full) {  // rare (one uniform branch): the tail, padded with zeros
#pragma unroll
            for (int l = 0; l < NLD; l++)
                pf[l] = load_unit<F>(in, hist, (long long)c * (PB * P) + (long long)sizeof(Raw) * (tid + l * NT), total, hb);
        }
        uint32_t ph = addmod(pc, rp.tid, N);
#pragma unroll
        for (int l = 0; l < NLD; l++) {
            const int u = tid + l * NT;
            stage_unit<D, F>(xb, H + 2 * u, pf[l], rot[ph], rot[addmod(ph, k, N)]);
            ph = addmod(ph, rp.ld, N);
        }
        pc = addmod(pc, rp.chunk, N);
        wave_sync();  // (A) chunk c staged
        if (c + 1 < c1) fetch(c + 1);

        // ---- low-pass + decimate: lane t owns outputs m = t + NT r; ascending k, one sequential sum
        float2v acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = float2v{0.0f, 0.0f};
        // Taps in groups of kG; a group's samples and taps are loaded while the group before it is
        // summed (two register sets; the scheduling barrier keeps the loads of later groups from
        // piling up in registers).  Tap kk = D j + i reads row (-i) mod D, column 16 + m - j - (i > 0).
        float2 X[2][kG][R];
        float hk[2][kG];
        auto ld = [&](int g) {
#pragma unroll
            for (int t = 0; t < kG; t++) {
                const int kk = g * kG + t;
                if (kk < C::T) {
                    const int i = kk % D, j = kk / D;
                    const float2* row = xb + ((D - i) % D) * W + (16 - j - (i > 0 ? 1 : 0)) + tid;
                    hk[g & 1][t] = h[kk];
#pragma unroll
                    for (int r = 0; r < R; r++) X[g & 1][t][r] = row[NT * r];
                }
            }
        };
        ld(0);
#pragma unroll
        for (int g = 0; g < C::NGRP; g++) {
            if (g + 1 < C::NGRP) ld(g + 1);
#pragma unroll
            for (int t = 0; t < kG; t++) {
                if (g * kG + t < C::T) {
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const float2 q = X[g & 1][t][r];
                        const float2v p = float2v{q.x, q.y} * hk[g & 1][t];
                        acc[r] = acc[r] + p;
                    }
                }
            }
            // the sums of a group stay in front of the next group's loads (and of the hand-off below)
#pragma unroll
            for (int r = 0; r < R; r++) asm volatile("" : "+v"(acc[r]));
            __builtin_amdgcn_sched_barrier(0);
        }
        wave_sync();  // (B) all reads of the chunk done

        // ---- the chunk's last H pairs (columns [CM, CM + 16) of every row) are the next one's history
        if (c + 1 < c1) {
#pragma unroll
            for (int i0 = 0; i0 < H; i0 += NT) {
                const int i = i0 + tid;
                if (i < H) xb[(i / 16) * W + (i % 16)] = xb[(i / 16) * W + CM + (i % 16)];
            }
        }
        const long long m0 = (long long)c * CM + tid;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const long long m = m0 + NT * r;
            if (m < n_out) yrow[m] = make_float2(acc[r].x, acc[r].y);
        }
    }
}

template <int D, int F>
int launch_one(const DdcLaunch& L, int n_streams, hipStream_t s) {
    hipLaunchKernelGGL((wide_ddc_kernel<D, F>), dim3(n_streams * L.segs), dim3(kNT), 0, s, L,
                       static_cast<const float*>(L.taps));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <int D>
int launch_decim(const DdcLaunch& L, int n_streams, hipStream_t s) {
    switch (L.format) {
        case kIqU8: return launch_one<D, kIqU8>(L, n_streams, s);
        case kIqS8: return launch_one<D, kIqS8>(L, n_streams, s);
        case kIqS16: return launch_one<D, kIqS16>(L, n_streams, s);
        case kIqF32: return launch_one<D, kIqF32>(L, n_streams, s);
    }
    return -1;
}

}  // namespace

int launch_decim_kernel(const DdcLaunch& L, int n_streams, hipStream_t s) {
    switch (L.down) {
        case 2: return launch_decim<2>(L, n_streams, s);
        case 3: return launch_decim<3>(L, n_streams, s);
        case 4: return launch_decim<4>(L, n_streams, s);
        case 5: return launch_decim<5>(L, n_streams, s);
        case 6: return launch_decim<6>(L, n_streams, s);
        case 7: return launch_decim<7>(L, n_streams, s);
        case 8: return launch_decim<8>(L, n_streams, s);
        case 9: return launch_decim<9>(L, n_streams, s);
        case 10: return launch_decim<10>(L, n_streams, s);
    }
    return -1;
}

}  // namespace fmrx
