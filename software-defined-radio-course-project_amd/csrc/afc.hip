// afc.hip — the carrier sums: per stream and 64 ms frame of a demod row, S = the sum of
// d[n] and Q = the sum of fl(d[n] d[n]), in the meter's shape.  Stateless: a frame depends on its own 64 P
// samples, so one workgroup takes one frame of one stream.  Per window, x = d[window start + n]:
//
//   a_j = fl(a_j + x[16 i + j]),  b_j = fl(b_j + fl(x[16 i + j] x[16 i + j])),  i ascending, j = 0..15
//   a_j = fl(a_j + a_{j+s}), s = 8, 4, 2, 1 (b alike);  the frame's 64 window values folded by the same tree, s = 32 .. 1
//
// Four lanes own a window: lane q of them loads the float4 at 16 i + 4 q for every i and so holds partials
// 4 q .. 4 q + 3 (64 B a window and load, every byte of the row read once, 16 B a lane).  All P / 16 loads
// of a lane are independent and issued before the first sum, 15 to 18 KiB a wave in flight.  The s = 8 and
// s = 4 folds are __shfl_down by 2 and by 1 over the four lanes (lane q adds what lane q + s / 4 holds: the
// definition's order), s = 2 and s = 1 stay inside lane 0 of the four.  The 64 window values cross the four
// waves through LDS and the first wave folds them as the meter does; lanes past a fold's width compute
// values nobody reads.  No tables, no atomics; lane 0 writes the frame's two floats.  Built without FP
// contraction.
#include <hip/hip_runtime.h>

#include "fmrx_internal.h"

namespace fmrx {

namespace {

constexpr int kThreads = 256;
static_assert(kMeterWindows * 4 == kThreads, "four lanes a window, one frame a workgroup");

template <int NI>
__global__ void __launch_bounds__(kThreads) carrier_kernel(CarrierLaunch L, int s0) {
    constexpr int P = 16 * NI;
    __shared__ float win[2][kMeterWindows];
    const int tid = threadIdx.x;
    const size_t s = (size_t)s0 + blockIdx.y, f = blockIdx.x;
    const int w = tid >> 2, q = tid & 3;
    const float4* x0 = reinterpret_cast<const float4*>(L.demod + s * L.demod_stride + (f * kMeterWindows + (size_t)w) * P) + q;
    float4 x[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) x[i] = x0[4 * i];
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const float v[4] = {x[i].x, x[i].y, x[i].z, x[i].w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float p = v[k] * v[k];
            a[k] = a[k] + v[k];
            b[k] = b[k] + p;
        }
    }
#pragma unroll
    for (int sh = 2; sh >= 1; sh >>= 1)  // s = 8, 4: partial j + s sits sh = s / 4 lanes up
#pragma unroll
        for (int k = 0; k < 4; k++) {
            a[k] = a[k] + __shfl_down(a[k], sh, 4);
            b[k] = b[k] + __shfl_down(b[k], sh, 4);
        }
    if (q == 0) {  // s = 2, 1
        const float a0 = a[0] + a[2], a1 = a[1] + a[3], b0 = b[0] + b[2], b1 = b[1] + b[3];
        win[0][w] = a0 + a1;
        win[1][w] = b0 + b1;
    }
    __syncthreads();
    if (tid < kMeterWindows) {  // the first wave: lane w holds window w's sums
        float va = win[0][tid], vb = win[1][tid];
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            va = va + __shfl_down(va, sh, 64);
            vb = vb + __shfl_down(vb, sh, 64);
        }
        if (tid == 0) *reinterpret_cast<float2*>(L.sums + (s * (size_t)L.frames + f) * 2) = make_float2(va, vb);
    }
}

}  // namespace

int launch_carrier(const CarrierLaunch& L, int n_streams, hipStream_t s) {
    if (L.frames == 0 || n_streams <= 0) return 0;
    if (L.frames < 0 || !L.demod || !L.sums) return -1;
    if (L.demod_stride < (size_t)L.frames * kMeterWindows * (size_t)L.P) return -1;
    // the lanes load float4: every row 16-byte aligned (a window is a multiple of 16 floats); the result float2
    if (reinterpret_cast<uintptr_t>(L.demod) % 16 != 0 || L.demod_stride % 4 != 0) return -1;
    if (reinterpret_cast<uintptr_t>(L.sums) % 8 != 0) return -1;
    for (int s0 = 0; s0 < n_streams; s0 += 65535) {  // grid.y holds the streams
        const int ny = n_streams - s0 < 65535 ? n_streams - s0 : 65535;
        const dim3 grid((unsigned)L.frames, (unsigned)ny), block(kThreads);
        switch (L.P) {
            case 240: hipLaunchKernelGGL(carrier_kernel<15>, grid, block, 0, s, L, s0); break;
            case 256: hipLaunchKernelGGL(carrier_kernel<16>, grid, block, 0, s, L, s0); break;
            case 288: hipLaunchKernelGGL(carrier_kernel<18>, grid, block, 0, s, L, s0); break;
            default: return -1;  // no mode has another window
        }
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace fmrx
