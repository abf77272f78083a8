// deemph.hip — FM de-emphasis in front of the S16 quantiser.  The one-pole filter of a
// 50 or 75 us time constant is, to float32 precision, a 64-tap FIR at the audio rates (p^64 < 2^-25),
// and a FIR is exact in parallel.  Per row (a stream's channel):
//
//   y[n] = sum_k h[k] x[n - k],  acc = fl(acc + fl(h[k] x)) from 0, k ascending   (filter.cpp:84-92
//                                                                                  with up = down = 1)
//   pcm[n] = quantize_s16(y[n])                                                    (project.cpp:185-191)
//
// with the 63 inputs in front of a call carried per row.  A workgroup takes kDeemphChunk outputs of one
// row: their inputs and the 63 before them go to LDS once, each lane reads the 67 floats its four
// consecutive outputs need as 17 ds_read_b128 and keeps them in registers.  The taps are a
// `const __restrict__` kernel-argument pointer read at constant indices: scalar loads, no VGPR.  The
// carry is double-buffered: the row's last workgroup writes the next call's 63 inputs from its LDS
// image into state_out while a first workgroup may still read state_in.
#include <hip/hip_runtime.h>

#include "dsp_device.h"
#include "fmrx_internal.h"

namespace fmrx {

namespace {

constexpr int kThreads = 256;
constexpr int kPer = kDeemphChunk / kThreads;        // consecutive outputs a lane
constexpr int kImage = kDeemphChunk + kDeemphTaps;   // floats staged: 63 of history, the chunk, one of padding
static_assert(kPer == 4, "a lane's outputs start on a float4 of the LDS image");
static_assert(kDeemphTaps % 4 == 0, "whole float4 reads");

__global__ void __launch_bounds__(kThreads) deemph_kernel(DeemphLaunch L, const float* __restrict__ h, int row0) {
    __shared__ float4 X4[kImage / 4];  // X[i]: sample c0 - 63 + i of the row (0 past its end)
    float* X = reinterpret_cast<float*>(X4);
    const int tid = threadIdx.x;
    const int row = row0 + (int)blockIdx.y;
    const int s = row / L.nch, ch = row - s * L.nch;
    const size_t c0 = (size_t)blockIdx.x * kDeemphChunk;
    const float* in = L.in + (size_t)s * L.in_stride + ch;
    const float* st = L.state_in + (size_t)row * kDeemphHist;
    for (int i = tid; i < kImage; i += kThreads) {
        const long long g = (long long)c0 + i - kDeemphHist;
        float v = 0.0f;
        if (g < 0) v = st[kDeemphHist + g];  // only the first chunk: g >= -63
        else if ((size_t)g < L.n) v = in[(size_t)g * L.nch];
        X[i] = v;
    }
    __syncthreads();
    // outputs 4 tid + r, r < 4: x[j] = X[4 tid + j], output r reads x[r + 63 - k] at tap k
    float x[kDeemphTaps + 4];
#pragma unroll
    for (int q = 0; q < kDeemphTaps / 4 + 1; q++) {
        const float4 v = X4[tid + q];
        x[4 * q] = v.x;
        x[4 * q + 1] = v.y;
        x[4 * q + 2] = v.z;
        x[4 * q + 3] = v.w;
    }
    float acc[kPer] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kDeemphTaps; k++) {
        const float hk = h[k];
#pragma unroll
        for (int r = 0; r < kPer; r++) {
            const float p = hk * x[r + kDeemphHist - k];
            acc[r] = acc[r] + p;
        }
    }
#pragma unroll
    for (int r = 0; r < kPer; r++) {
        const size_t o = c0 + (size_t)(kPer * tid + r);
        if (o >= L.n) continue;
        const size_t at = (size_t)s * L.out_stride + ch + o * L.nch;
        if (L.out) L.out[at] = acc[r];
        if (L.pcm) L.pcm[at] = quantize_s16(acc[r]);
    }
    // the next call's history: the last 63 of (history ++ input), all inside the last chunk's image
    if (blockIdx.x == gridDim.x - 1 && tid < kDeemphHist)
        L.state_out[(size_t)row * kDeemphHist + tid] = X[(L.n - c0) + tid];
}

}  // namespace

int launch_deemph(const DeemphLaunch& L, int n_streams, hipStream_t s) {
    if (L.n == 0 || n_streams <= 0) return 0;
    if (L.nch < 1 || L.nch > 2 || L.state_in == L.state_out) return -1;
    const size_t chunks = (L.n + kDeemphChunk - 1) / kDeemphChunk;
    if (chunks > 0x7FFFFFFFull) return -1;
    const int rows = n_streams * L.nch;
    for (int row0 = 0; row0 < rows; row0 += 65535) {  // grid.y holds stream x channel
        const int ny = rows - row0 < 65535 ? rows - row0 : 65535;
        hipLaunchKernelGGL(deemph_kernel, dim3((unsigned)chunks, (unsigned)ny), dim3(kThreads), 0, s, L, L.h, row0);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace fmrx
