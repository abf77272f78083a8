// meter.hip — the subcarrier meter: per stream and 64 ms frame, the power of the demod
// row at seven tones (17, 19, 21, 56, 58, 61, 63 kHz) through Hann-windowed 1 ms DFT bins.  Stateless:
// a frame depends on its own 64 P samples, so one workgroup takes one frame of one stream and nothing
// loops over frames in time.  Per window and table row (tone-major, c then s; include/fmrx.h):
//
//   a_j = fl(a_j + fl(x[16 i + j] tab[16 i + j])), i ascending, j = 0..15;  a_j = fl(a_j + a_{j+s}), s = 8, 4, 2, 1
//   p = fl(fl(re re) + fl(im im));  the frame's 64 window powers folded by the same tree, s = 32 .. 1
//
// A 16-lane group owns four consecutive windows: lane j reads samples 16 i + j of each (64 B a group and
// load, every byte of the row read once) and keeps the 14 x 4 partial sums in registers, so one LDS
// read of a table entry serves four windows.  The 14 tables (at most 16,128 B) are staged in LDS once a
// workgroup; the four groups of a wave read the same addresses (a broadcast, no bank conflict).  The
// folds are __shfl_down over 16 and 64 lanes: lane j adds what lane j + s holds, which is the definition's
// order; lanes past the fold's width compute values nobody reads.  Built without FP contraction.
#include <hip/hip_runtime.h>

#include "fmrx_internal.h"

namespace fmrx {

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 2 * kMeterTones;                        // table rows: c and s of every tone
constexpr int kPerGroup = kMeterWindows / (kThreads / 16);    // windows a 16-lane group
static_assert(kPerGroup == 4, "four windows a group share one table read");
static_assert(kMeterWindows == 64, "the frame fold is one wave wide");

template <int NI>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) meter_kernel(MeterLaunch L, int s0) {
    constexpr int P = 16 * NI;
    __shared__ float4 T4[kRows * P / 4];
    __shared__ float pw[kMeterTones][kMeterWindows];
    const float* T = reinterpret_cast<const float*>(T4);
    const int tid = threadIdx.x;
    const float4* src = reinterpret_cast<const float4*>(L.tables);
    for (int i = tid; i < kRows * P / 4; i += kThreads) T4[i] = src[i];
    const size_t s = (size_t)s0 + blockIdx.y, f = blockIdx.x;
    const int g = tid >> 4, j = tid & 15;
    const float* x0 = L.demod + s * L.demod_stride + (f * kMeterWindows + (size_t)(kPerGroup * g)) * P + j;
    __syncthreads();
    float acc[kRows][kPerGroup];
#pragma unroll
    for (int t = 0; t < kRows; t++)
#pragma unroll
        for (int q = 0; q < kPerGroup; q++) acc[t][q] = 0.0f;
    // kStep values of i a trip: their 4 kStep loads are issued together, and the 56 sums, the loads and the
    // addresses stay within 128 VGPRs without scratch (a longer trip spills), so four waves a SIMD hide the
    // loads' latency behind each other's sums
    constexpr int kStep = NI % 3 == 0 ? 3 : 2;
    static_assert(NI % kStep == 0, "whole trips");
#pragma unroll 1
    for (int i0 = 0; i0 < NI; i0 += kStep) {
        float x[kStep][kPerGroup];
#pragma unroll
        for (int u = 0; u < kStep; u++)
#pragma unroll
            for (int q = 0; q < kPerGroup; q++) x[u][q] = x0[q * P + 16 * (i0 + u)];
#pragma unroll
        for (int u = 0; u < kStep; u++)
#pragma unroll
            for (int t = 0; t < kRows; t++) {
                const float c = T[t * P + 16 * (i0 + u) + j];
#pragma unroll
                for (int q = 0; q < kPerGroup; q++) {
                    const float p = x[u][q] * c;
                    acc[t][q] = acc[t][q] + p;
                }
            }
    }
#pragma unroll
    for (int sh = 8; sh >= 1; sh >>= 1)
#pragma unroll
        for (int t = 0; t < kRows; t++)
#pragma unroll
            for (int q = 0; q < kPerGroup; q++) acc[t][q] = acc[t][q] + __shfl_down(acc[t][q], sh, 16);
    if (j == 0) {
#pragma unroll
        for (int k = 0; k < kMeterTones; k++)
#pragma unroll
            for (int q = 0; q < kPerGroup; q++) {
                const float rr = acc[2 * k][q] * acc[2 * k][q];
                const float ii = acc[2 * k + 1][q] * acc[2 * k + 1][q];
                pw[k][kPerGroup * g + q] = rr + ii;
            }
    }
    __syncthreads();
    if (tid < kMeterWindows) {  // the first wave: lane w holds window w's power
        float* out = L.power + (s * (size_t)L.frames + f) * kMeterTones;
#pragma unroll
        for (int k = 0; k < kMeterTones; k++) {
            float v = pw[k][tid];
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) v = v + __shfl_down(v, sh, 64);
            if (tid == 0) out[k] = v;
        }
    }
}

}  // namespace

int launch_meter(const MeterLaunch& L, int n_streams, hipStream_t s) {
    if (L.frames == 0 || n_streams <= 0) return 0;
    if (L.frames < 0 || !L.demod || !L.tables || !L.power) return -1;
    if (L.demod_stride < (size_t)L.frames * kMeterWindows * (size_t)L.P) return -1;
    if (reinterpret_cast<uintptr_t>(L.tables) % 16 != 0) return -1;
    for (int s0 = 0; s0 < n_streams; s0 += 65535) {  // grid.y holds the streams
        const int ny = n_streams - s0 < 65535 ? n_streams - s0 : 65535;
        const dim3 grid((unsigned)L.frames, (unsigned)ny), block(kThreads);
        switch (L.P) {
            case 240: hipLaunchKernelGGL(meter_kernel<15>, grid, block, 0, s, L, s0); break;
            case 256: hipLaunchKernelGGL(meter_kernel<16>, grid, block, 0, s, L, s0); break;
            case 288: hipLaunchKernelGGL(meter_kernel<18>, grid, block, 0, s, L, s0); break;
            default: return -1;  // no mode has another window
        }
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace fmrx
