// scan.hip — the band scan's spectrum: Welch power spectrum of a raw I/Q capture (u8, s8, s16, f32)
// (fmrx_scan_spectrum*).  A floating-point estimate, checked against numpy
// float64 to a stated tolerance (tests/test_gpu_scan.py); the same input gives the same bits
// on every run (no atomics, fixed summation order).
//
//   scan_segments_kernel<L, F>  N = 2^L, F the raw format (ScanFmt below).
//                            Workgroup g walks segments g, g + G, ...: coalesced loads of two
//                            pairs a lane (a dword of u8 / s8, the next segment's in flight during the
//                            transform), integer sample * window into LDS as complex float, an in-place
//                            decimation-in-frequency FFT -- one radix-2/4/8 pass when L is no
//                            multiple of 4, then radix-16 passes, every butterfly in registers and
//                            one LDS round trip a pass -- whose last pass adds |X|^2 to registers
//                            instead of storing.  The outputs stay in digit-reversed order until
//                            the workgroup writes its one partial row of N floats.
//   scan_reduce_kernel       sums the partial rows in a fixed order in double, scales and shifts.
//
// LDS image: element i at i + i / 16 (one pad element every 16).  The pass of sub-length M = 16
// reads 16 consecutive elements a lane (17-element lane stride: the 32 lanes of a ds_read_b64
// group on 32 distinct bank pairs), the pass of M = 256 reads runs of 16 a block (272-element
// block stride: the two halves of the 256-B bank row); the first pass's runs of 32 straddle one pad
// (one 2-way pair a group).  Stores go in runs of 16 consecutive elements, conflict-free.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "scan.h"
#include "tuner.h"

namespace fmrx {

namespace {

constexpr int kScanThreads = 256;

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// explicit fused multiply-adds (the package builds with -ffp-contract=off: nothing contracts by itself)
__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
    return make_float2(fmaf(a.x, w.x, -(a.y * w.y)), fmaf(a.x, w.y, a.y * w.x));
}

// d * exp(-2 pi j E / 16)
template <int E>
__device__ __forceinline__ float2 rot16(float2 d) {
    constexpr float kR = 0.70710678118654752f, kC = 0.92387953251128674f, kS = 0.38268343236508977f;
    if constexpr (E == 0) {
        return d;
    } else if constexpr (E == 4) {
        return make_float2(d.y, -d.x);
    } else if constexpr (E == 2) {
        return make_float2(kR * (d.x + d.y), kR * (d.y - d.x));
    } else if constexpr (E == 6) {
        return make_float2(kR * (d.y - d.x), -(kR * (d.x + d.y)));
    } else {
        constexpr float c = E == 1 ? kC : E == 3 ? kS : E == 5 ? -kS : -kC;
        constexpr float s = (E == 1 || E == 7) ? kS : kC;
        return make_float2(fmaf(d.x, c, d.y * s), fmaf(d.y, c, -(d.x * s)));
    }
}

// v[p] <- sum_q v[q] exp(-2 pi j p q / R), natural order in and out, R in {1, 2, 4, 8, 16}
template <int R>
struct Dft {
    template <int Q>
    static __device__ __forceinline__ void split(const float2 (&v)[R], float2 (&a)[R / 2], float2 (&b)[R / 2]) {
        a[Q] = cadd(v[Q], v[Q + R / 2]);
        b[Q] = rot16<Q * (16 / R)>(csub(v[Q], v[Q + R / 2]));
        if constexpr (Q + 1 < R / 2) split<Q + 1>(v, a, b);
    }
    static __device__ __forceinline__ void run(float2 (&v)[R]) {
        float2 a[R / 2], b[R / 2];
        split<0>(v, a, b);
        Dft<R / 2>::run(a);
        Dft<R / 2>::run(b);
#pragma unroll
        for (int k = 0; k < R / 2; k++) {
            v[2 * k] = a[k];
            v[2 * k + 1] = b[k];
        }
    }
};
template <>
struct Dft<1> {
    static __device__ __forceinline__ void run(float2 (&)[1]) {}
};

__device__ __forceinline__ int padi(int i) { return i + (i >> 4); }

constexpr int scan_iters(int n) { return n / kScanThreads > 0 ? n / kScanThreads : 1; }

// table index of butterfly b's twiddle for output p of a radix-R pass of sub-length M
template <int N, int R, int M>
__device__ __forceinline__ int tw_index(int b, int p) {
    return ((b & (M / R - 1)) * p) * (N / M);
}

template <int N, int R, int M, int IT>
__device__ __forceinline__ void load_twiddles(const float2* __restrict__ tw, int tid, float2 (&twr)[IT][R - 1]) {
#pragma unroll
    for (int it = 0; it < IT; it++)
#pragma unroll
        for (int p = 1; p < R; p++) twr[it][p - 1] = tw[tw_index<N, R, M>(tid + it * kScanThreads, p)];
}

// One decimation-in-frequency pass over the N elements of buf: butterfly b takes the R elements
// j + q S of block b / S (S = M / R, j = b mod S), output p times exp(-2 pi j (j p) / M) goes back
// to j + p S.  PRE: the twiddles come from twr (loaded once a workgroup), else from the table.
template <int N, int R, int M, bool PRE, int IT>
__device__ __forceinline__ void scan_pass(float2* buf, int tid, const float2* __restrict__ tw,
                                          const float2 (&twr)[IT][R - 1]) {
    constexpr int S = M / R, NB = N / R;
    static_assert(S >= 16, "a storing pass keeps runs of 16");
#pragma unroll
    for (int it = 0; it < IT; it++) {
        const int b = tid + it * kScanThreads;
        if (NB % kScanThreads == 0 || b < NB) {
            const int at = padi((b / S) * M + (b & (S - 1)));
            float2 v[R];
#pragma unroll
            for (int q = 0; q < R; q++) v[q] = buf[at + q * (S + S / 16)];
            Dft<R>::run(v);
            buf[at] = v[0];
#pragma unroll
            for (int p = 1; p < R; p++) {
                const float2 w = PRE ? twr[it][p - 1] : tw[tw_index<N, R, M>(b, p)];
                buf[at + p * (S + S / 16)] = cmul(v[p], w);
            }
        }
    }
}

// The last pass (M = 16): butterfly b transforms elements 16 b .. 16 b + 15 and adds |X|^2 to acc.
template <int N, int IT>
__device__ __forceinline__ void scan_last(const float2* buf, int tid, float (&acc)[IT][16]) {
    constexpr int NB = N / 16;
#pragma unroll
    for (int it = 0; it < IT; it++) {
        const int b = tid + it * kScanThreads;
        if (NB % kScanThreads == 0 || b < NB) {
            float2 v[16];
#pragma unroll
            for (int q = 0; q < 16; q++) v[q] = buf[b * 17 + q];
            Dft<16>::run(v);
#pragma unroll
            for (int p = 0; p < 16; p++) acc[it][p] = fmaf(v[p].x, v[p].x, fmaf(v[p].y, v[p].y, acc[it][p]));
        }
    }
}

// Frequency index of the element the passes leave at position pos: pass radices R1, R2, ... and the
// position's digits p1, p2, ... (most significant first) give k = p1 + R1 (p2 + R2 (p3 + ...)).
template <int L>
__device__ __forceinline__ int scan_freq(int pos) {
    constexpr int R0 = 1 << (L & 3);
    int m = 1 << L, k = 0, mult = 1;
    if (R0 > 1) {
        m /= R0;
        k = pos / m;
        pos &= m - 1;
        mult = R0;
    }
    while (m > 1) {
        m /= 16;
        k += (pos / m) * mult;
        pos &= m - 1;
        mult *= 16;
    }
    return k;
}

// Dword d of the capture (pairs 2 d and 2 d + 1) from the 4-byte-aligned words around it: base is
// iq rounded down to 4 bytes, shift the bytes in between.  With shift != 0 the second word holds
// the dword's last bytes, so it lies inside the capture's last aligned word at the latest.
__device__ __forceinline__ uint32_t scan_dword(const uint32_t* __restrict__ base, unsigned shift, size_t d) {
    uint32_t w = base[d];
    if (shift) {
        const uint32_t hi = base[d + 1];
        w = (uint32_t)((((uint64_t)hi << 32) | w) >> (8 * shift));
    }
    return w;
}

// A raw format's unit of two I/Q pairs (Raw), how a unit is loaded and its samples as exact floats
// (i0, q0, i1, q1) times a power of two that launch_scan folds into the final scale.  u8 and s8
// share the dword layout and the funnel shift of a start on any pair; s16 and f32 pairs are
// always element-aligned (4 and 8 bytes), so they take plain loads of that alignment.
template <int F>
struct ScanFmt;
template <>
struct ScanFmt<kIqU8> {
    using Raw = uint32_t;
    static __device__ __forceinline__ Raw load(const uint8_t* iq, const uint32_t* base, unsigned shift, size_t d) {
        return scan_dword(base, shift, d);
    }
    static __device__ __forceinline__ float4 unpack(Raw w) {
        return make_float4((float)(w & 255u) - 128.0f, (float)((w >> 8) & 255u) - 128.0f,
                           (float)((w >> 16) & 255u) - 128.0f, (float)(w >> 24) - 128.0f);
    }
};
template <>
struct ScanFmt<kIqS8> {
    using Raw = uint32_t;
    static __device__ __forceinline__ Raw load(const uint8_t* iq, const uint32_t* base, unsigned shift, size_t d) {
        return scan_dword(base, shift, d);
    }
    static __device__ __forceinline__ float4 unpack(Raw w) { return ScanFmt<kIqU8>::unpack(w ^ 0x80808080u); }
};
template <>
struct ScanFmt<kIqS16> {
    using Raw = uint2;
    static __device__ __forceinline__ Raw load(const uint8_t* iq, const uint32_t*, unsigned, size_t d) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(iq) + 2 * d;  // a pair a dword
        return make_uint2(p[0], p[1]);
    }
    static __device__ __forceinline__ float4 unpack(Raw w) {
        return make_float4((float)((int)(w.x << 16) >> 16), (float)((int)w.x >> 16), (float)((int)(w.y << 16) >> 16),
                           (float)((int)w.y >> 16));
    }
};
template <>
struct ScanFmt<kIqF32> {
    using Raw = float4;
    static __device__ __forceinline__ Raw load(const uint8_t* iq, const uint32_t*, unsigned, size_t d) {
        const float2* p = reinterpret_cast<const float2*>(iq) + 2 * d;  // 8-byte aligned pairs
        const float2 a = p[0], b = p[1];
        return make_float4(a.x, a.y, b.x, b.y);
    }
    static __device__ __forceinline__ float4 unpack(Raw w) { return w; }
};

template <int L, int F>
__global__ void __launch_bounds__(kScanThreads)
scan_segments_kernel(const uint8_t* __restrict__ iq, unsigned nseg, const float2* __restrict__ tw,
                     const float2* __restrict__ win, float* __restrict__ part) {
    constexpr int N = 1 << L, T = kScanThreads;
    constexpr int R0 = 1 << (L & 3);        // the first pass's radix (1: none)
    constexpr int MA = N / R0;              // sub-length of the first radix-16 pass
    constexpr int N16 = L / 4;              // radix-16 passes, the last one included
    constexpr bool PRE = N <= 4096;         // twiddles and window in registers
    constexpr int DW = scan_iters(N / 2);   // units (two pairs) a thread loads per segment
    using Fmt = ScanFmt<F>;
    using Raw = typename Fmt::Raw;
    // the next segment's units stay in flight during the transform while they fit the 16 registers
    // the u8 kernel gives them at 8192 bins; a wider format past that loads at staging time
    constexpr bool PF = DW * (int)(sizeof(Raw) / 4) <= 16;
    constexpr int IT0 = scan_iters(N / (R0 > 1 ? R0 : 2)), IT16 = scan_iters(N / 16);
    static_assert(N16 == 2 || N16 == 3, "256 <= N <= 8192");
    __shared__ float2 buf[N + N / 16];

    const int tid = threadIdx.x;
    const unsigned shift = sizeof(Raw) == 4 ? (unsigned)(reinterpret_cast<uintptr_t>(iq) & 3u) : 0u;
    const uint32_t* base = reinterpret_cast<const uint32_t*>(iq - shift);

    float2 wv[DW];
    float2 tw0[IT0][R0 > 1 ? R0 - 1 : 1], twa[IT16][15], twb[IT16][15];
    if (PRE) {
#pragma unroll
        for (int it = 0; it < DW; it++) wv[it] = win[(tid + it * T) & (N / 2 - 1)];
        if constexpr (R0 > 1) load_twiddles<N, R0, N, IT0>(tw, tid, tw0);
        load_twiddles<N, 16, MA, IT16>(tw, tid, twa);
        if constexpr (N16 == 3) load_twiddles<N, 16, MA / 16, IT16>(tw, tid, twb);
    }
    float acc[IT16][16];
#pragma unroll
    for (int it = 0; it < IT16; it++)
#pragma unroll
        for (int p = 0; p < 16; p++) acc[it][p] = 0.0f;

    Raw raw[PF ? DW : 1];
    unsigned seg = blockIdx.x;
    if (PF && seg < nseg) {
#pragma unroll
        for (int it = 0; it < DW; it++) {
            const int d = tid + it * T;
            if ((N / 2) % T == 0 || d < N / 2) raw[it] = Fmt::load(iq, base, shift, (size_t)seg * (N / 2) + d);
        }
    }
    for (; seg < nseg; seg += gridDim.x) {
        // the integer sample is exact in float; the power of two of the normalisation (2^-7, 2^-15)
        // is folded into the final scale
#pragma unroll
        for (int it = 0; it < DW; it++) {
            const int d = tid + it * T;
            if ((N / 2) % T == 0 || d < N / 2) {
                const float4 x = Fmt::unpack(PF ? raw[it] : Fmt::load(iq, base, shift, (size_t)seg * (N / 2) + d));
                const float2 h = PRE ? wv[it] : win[d];
                const int at = padi(2 * d);
                buf[at] = make_float2(x.x * h.x, x.y * h.x);
                buf[at + 1] = make_float2(x.z * h.y, x.w * h.y);
            }
            // loads at staging time go four units at a time: hoisted together they would take the
            // registers the transform's twiddles and accumulators hold
            if (!PF && it % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
        const unsigned next = seg + gridDim.x;
        if (PF && next < nseg) {
#pragma unroll
            for (int it = 0; it < DW; it++) {
                const int d = tid + it * T;
                if ((N / 2) % T == 0 || d < N / 2) raw[it] = Fmt::load(iq, base, shift, (size_t)next * (N / 2) + d);
            }
        }
        __syncthreads();
        if constexpr (R0 > 1) {
            scan_pass<N, R0, N, PRE, IT0>(buf, tid, tw, tw0);
            __syncthreads();
        }
        scan_pass<N, 16, MA, PRE, IT16>(buf, tid, tw, twa);
        __syncthreads();
        if constexpr (N16 == 3) {
            scan_pass<N, 16, MA / 16, PRE, IT16>(buf, tid, tw, twb);
            __syncthreads();
        }
        scan_last<N, IT16>(buf, tid, acc);
        __syncthreads();  // the next segment's samples overwrite buf
    }
    float* row = part + (size_t)blockIdx.x * N;
#pragma unroll
    for (int it = 0; it < IT16; it++) {
        const int b = tid + it * T;
        if ((N / 16) % T == 0 || b < N / 16) {
#pragma unroll
            for (int p = 0; p < 16; p++) row[scan_freq<L>(b * 16 + p)] = acc[it][p];
        }
    }
}

// power[j] = scale * sum over the G partial rows of bin (j - N/2) mod N, in double and in a fixed
// order: a workgroup takes 64 bins; slice t of its 16 adds rows t, t + 16, ... in row order, then
// the slices' sums are added in slice order.
constexpr int kReduceBins = 64, kReduceSlices = 16;
__global__ void __launch_bounds__(kReduceBins * kReduceSlices)
scan_reduce_kernel(const float* __restrict__ part, int G, int N, double scale, float* __restrict__ power) {
    __shared__ double sums[kReduceSlices][kReduceBins];
    const int lane = threadIdx.x % kReduceBins, slice = threadIdx.x / kReduceBins;
    const int j = blockIdx.x * kReduceBins + lane;  // N is a multiple of 64
    const int k = j ^ (N / 2);
    double sum = 0.0;
    for (int g = slice; g < G; g += kReduceSlices) sum += (double)part[(size_t)g * N + k];
    sums[slice][lane] = sum;
    __syncthreads();
    if (slice == 0) {
        double total = 0.0;
#pragma unroll
        for (int t = 0; t < kReduceSlices; t++) total += sums[t][lane];
        power[j] = (float)(total * scale);
    }
}

template <int L, int F>
int scan_occupancy_format(int* per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, scan_segments_kernel<L, F>, kScanThreads, 0) == hipSuccess
               ? 0 : -2;
}

template <int L>
int scan_occupancy(int format, int* per_cu) {
    switch (format) {
        case kIqU8: return scan_occupancy_format<L, kIqU8>(per_cu);
        case kIqS8: return scan_occupancy_format<L, kIqS8>(per_cu);
        case kIqS16: return scan_occupancy_format<L, kIqS16>(per_cu);
        case kIqF32: return scan_occupancy_format<L, kIqF32>(per_cu);
    }
    return -2;
}

template <int L, int F>
void scan_launch_format(const uint8_t* iq, unsigned nseg, const float* tw, const float* win, float* part, int G,
                        hipStream_t s) {
    hipLaunchKernelGGL((scan_segments_kernel<L, F>), dim3(G), dim3(kScanThreads), 0, s, iq, nseg,
                       reinterpret_cast<const float2*>(tw), reinterpret_cast<const float2*>(win), part);
}

template <int L>
void scan_launch(int format, const uint8_t* iq, unsigned nseg, const float* tw, const float* win, float* part, int G,
                 hipStream_t s) {
    switch (format) {
        case kIqU8: scan_launch_format<L, kIqU8>(iq, nseg, tw, win, part, G, s); break;
        case kIqS8: scan_launch_format<L, kIqS8>(iq, nseg, tw, win, part, G, s); break;
        case kIqS16: scan_launch_format<L, kIqS16>(iq, nseg, tw, win, part, G, s); break;
        case kIqF32: scan_launch_format<L, kIqF32>(iq, nseg, tw, win, part, G, s); break;
    }
}

int scan_log2(int N) {
    int l = 0;
    while ((1 << l) < N) l++;
    return l;
}

}  // namespace

void scan_tables(int N, float* tw, float* win) {
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < N; k++) {
        const double a = two_pi * (double)k / (double)N;
        tw[2 * k] = (float)std::cos(a);
        tw[2 * k + 1] = (float)-std::sin(a);
        win[k] = (float)(0.5 - 0.5 * std::cos(a));
    }
}

int scan_workgroups(int N, size_t nseg, int cus, int format) {
    if (!scan_bins_ok(N) || nseg < 1 || iq_pair_bytes(format) < 0) return 0;
    int per_cu = 0, rc = -2;
    switch (scan_log2(N)) {
        case 8: rc = scan_occupancy<8>(format, &per_cu); break;
        case 9: rc = scan_occupancy<9>(format, &per_cu); break;
        case 10: rc = scan_occupancy<10>(format, &per_cu); break;
        case 11: rc = scan_occupancy<11>(format, &per_cu); break;
        case 12: rc = scan_occupancy<12>(format, &per_cu); break;
        case 13: rc = scan_occupancy<13>(format, &per_cu); break;
    }
    if (rc || per_cu < 1) return 0;
    const size_t resident = (size_t)(cus > 0 ? cus : 1) * (size_t)per_cu;
    return (int)(nseg < resident ? nseg : resident);
}

int launch_scan(const uint8_t* iq, int format, size_t nseg, int N, const float* d_tw, const float* d_win, float* d_part,
                int G, float* d_power, hipStream_t s) {
    if (!scan_bins_ok(N) || nseg < 1 || nseg > 0xffffffffu || G < 1 || (size_t)G > nseg) return -1;
    if (iq_pair_bytes(format) < 0) return -1;
    const unsigned ns = (unsigned)nseg;
    switch (scan_log2(N)) {
        case 8: scan_launch<8>(format, iq, ns, d_tw, d_win, d_part, G, s); break;
        case 9: scan_launch<9>(format, iq, ns, d_tw, d_win, d_part, G, s); break;
        case 10: scan_launch<10>(format, iq, ns, d_tw, d_win, d_part, G, s); break;
        case 11: scan_launch<11>(format, iq, ns, d_tw, d_win, d_part, G, s); break;
        case 12: scan_launch<12>(format, iq, ns, d_tw, d_win, d_part, G, s); break;
        case 13: scan_launch<13>(format, iq, ns, d_tw, d_win, d_part, G, s); break;
    }
    // P = 8 / (3 N^2 nseg) sum |FFT(w x)|^2 with x the integer sample times 2^-7 (u8, s8) or 2^-15
    // (s16): the folded square of that power of two; none for f32
    const double fold = format == kIqF32 ? 1.0 : format == kIqS16 ? 1073741824.0 : 16384.0;
    const double scale = 8.0 / (3.0 * (double)N * (double)N * (double)nseg) / fold;
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(N / kReduceBins), dim3(kReduceBins * kReduceSlices), 0, s, d_part, G, N,
                       scale, d_power);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace fmrx
