// rds_bits.hip — RDS back half: the 57 kHz mixer output of rds.hip to differential
// bits and block syndromes.  Per stream, over whole windows of kRdsbWin outputs:
//
//   y[n]   = resample(m, h, 19, down)          38 kS/s, the reference's resample (filter.cpp:67-103)
//   s[n]   = y[n] >= 0                         the only use of a float past this line
//   p_w    = (argmax_z #{n in window w : s[n] != s[n-1], n mod 16 = z} + 8) mod 16
//   c_w[j] = s[2432 w + p_w + 16 j]            152 biphase chips a window
//   q_w    = pairing vote, d = 76 symbols      first chip of each pair
//   bit[i] = d[i] ^ d[i-1],  code[i] = offset word the syndrome of bits i-25..i equals (0: none)
//
// Nothing is serial in time: every kernel runs one workgroup (or lane) per window (or bit) and
// stream.  A window starts at input 128 down w with phase 0 (2432 = 128 x 19), so a chunk of 608
// outputs reads 32 down inputs and 100 of history, staged once in LDS; all 19 phases hold exactly
// 101 taps (1919 = 101 x 19) and the sum keeps filter.cpp:84-92's order (k ascending, products
// rounded separately, the build has no contraction).
#include <hip/hip_runtime.h>

#include "fmrx_internal.h"

namespace fmrx {

namespace {

constexpr int kUp = kRdsbUp;
constexpr int kPT = kRdsbPhaseTaps;          // taps a phase
constexpr int kBack = kPT - 1;               // inputs an output reads before its base
constexpr int kPeriods = 32;                 // input periods (down inputs, 19 outputs) a chunk
constexpr int kChunkOut = kPeriods * kUp;    // 608 outputs; a window is 4 chunks
constexpr int kMaxDown = 144;
constexpr int kResThreads = 320;             // two outputs a lane (608 <= 640)
static_assert(kRdsbWin % kChunkOut == 0, "a window is whole chunks");
static_assert(kRdsbHist >= kBack, "the carried inputs cover a phase's taps");

__global__ void __launch_bounds__(kResThreads) rdsb_resample_kernel(RdsBitsLaunch L) {
    __shared__ float xs[kPeriods * kMaxDown + kBack];  // inputs [ib - 100, ib + 32 down)
    __shared__ float hs[kRdsbTaps];
    const int tid = threadIdx.x;
    const int s = blockIdx.y;
    const int down = L.down;
    const int n_in = kPeriods * down;
    const int ib = blockIdx.x * n_in;  // < n_if
    const float* m = L.mix + (size_t)s * L.mix_stride;
    const float* hist = L.hist + (size_t)s * kRdsbHist;  // the kRdsbHist inputs before m[0]
    for (int i = tid; i < kRdsbTaps; i += kResThreads) hs[i] = L.taps[i];
    for (int i = tid; i < n_in + kBack; i += kResThreads) {
        const int j = ib - kBack + i;  // j < ib + n_in <= n_if
        xs[i] = j < 0 ? hist[kRdsbHist + j] : m[j];
    }
    __syncthreads();
    for (int t = tid; t < kChunkOut; t += kResThreads) {
        const int nd = t * down;
        const int j0 = nd / kUp;
        const int k0 = nd - j0 * kUp;
        const float* x = xs + kBack + j0;  // x[-100 .. 0] inside xs: j0 <= 32 down - 1
        const float* h = hs + k0;          // k0 + 19 x 100 <= 1918
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < kPT; i++) {
            const float p = h[i * kUp] * x[-i];
            acc = acc + p;
        }
        const size_t n = (size_t)blockIdx.x * kChunkOut + t;
        if (L.y) L.y[(size_t)s * L.n_out + n] = acc;
        L.sign[(size_t)s * L.n_out + n] = acc >= 0.0f ? 1 : 0;
    }
}

// One workgroup a window: sign changes by n mod 16 (256 = 16 x 16 lanes, so a lane stays in one
// bin), the phase, and the window's last chip for its successor's pairing.
__global__ void __launch_bounds__(256) rdsb_phase_kernel(RdsBitsLaunch L) {
    __shared__ int bins[16];
    const int tid = threadIdx.x;
    const int w = blockIdx.x, s = blockIdx.y;
    const uint8_t* sg = L.sign + (size_t)s * L.n_out + (size_t)w * kRdsbWin;
    if (tid < 16) bins[tid] = 0;
    __syncthreads();
    int cnt = 0;
    for (int n = tid; n < kRdsbWin; n += 256) {
        // the sample in front of the window: its predecessor's last, or the carried one
        const uint8_t prev = (n == 0 && w == 0) ? L.state[(size_t)s * kRdsbStateBytes + 0] : sg[n - 1];
        cnt += sg[n] != prev;
    }
    atomicAdd(&bins[tid & 15], cnt);
    __syncthreads();
    if (tid == 0) {
        int z = 0;
        for (int k = 1; k < 16; k++)
            if (bins[k] > bins[z]) z = k;  // the lowest index of the largest bin
        const int p = (z + 8) & 15;
        L.winp[(size_t)s * L.n_win + w] = (uint8_t)p;
        L.lastchip[(size_t)s * L.n_win + w] = sg[p + 16 * (kRdsbChips - 1)];  // <= 15 + 2416 < 2432
    }
}

// One workgroup a window, one lane a chip pair: the pairing vote and the 76 symbols.
__global__ void __launch_bounds__(128) rdsb_symbol_kernel(RdsBitsLaunch L) {
    __shared__ int votes[2];
    const int i = threadIdx.x;
    const int w = blockIdx.x, s = blockIdx.y;
    const uint8_t* sg = L.sign + (size_t)s * L.n_out + (size_t)w * kRdsbWin;
    if (i < 2) votes[i] = 0;
    __syncthreads();
    const int p = L.winp[(size_t)s * L.n_win + w];
    uint8_t a = 0, b = 0;
    if (i < kRdsbSyms) {
        // e[0] = the chip in front of the window, e[k] = c_w[k - 1]
        const uint8_t e0 = w == 0 ? L.state[(size_t)s * kRdsbStateBytes + 1] : L.lastchip[(size_t)s * L.n_win + w - 1];
        a = i == 0 ? e0 : sg[p + 16 * (2 * i - 1)];
        b = sg[p + 16 * (2 * i)];
        const uint8_t c = sg[p + 16 * (2 * i + 1)];  // chip 2 i + 1 <= 151
        if (a == b) atomicAdd(&votes[0], 1);
        if (b == c) atomicAdd(&votes[1], 1);
    }
    __syncthreads();
    const int q = votes[1] <= votes[0] ? 0 : 1;
    if (i < kRdsbSyms) L.sym[(size_t)s * L.n_sym + (size_t)w * kRdsbSyms + i] = q ? a : b;
    if (i == 0 && L.win) {
        L.win[((size_t)s * L.n_win + w) * 2 + 0] = (uint8_t)p;
        L.win[((size_t)s * L.n_win + w) * 2 + 1] = (uint8_t)q;
    }
}

// One lane a bit: the differential bit and the syndrome of the 26 bits ending at it.  The
// remainder of the whole word by the generator equals crc10(info) ^ check.
__global__ void __launch_bounds__(256) rdsb_code_kernel(RdsBitsLaunch L) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= L.n_sym) return;
    const uint8_t* sym = L.sym + (size_t)s * L.n_sym;
    const uint8_t* st = L.state + (size_t)s * kRdsbStateBytes;
    auto d = [&](int k) -> unsigned { return k >= 0 ? sym[k] : st[4 + kRdsbTail + k]; };  // k >= -26
    unsigned prev = d(i - 26), reg = 0, bit = 0;
    for (int k = i - 25; k <= i; k++) {
        const unsigned cur = d(k);
        bit = cur ^ prev;
        prev = cur;
        reg = (reg << 1) | bit;
        if (reg & 0x400u) reg ^= 0x5B9u;
    }
    unsigned code = 0;
    if (reg == 0x0FCu) code = 1;
    else if (reg == 0x198u) code = 2;
    else if (reg == 0x168u) code = 3;
    else if (reg == 0x350u) code = 4;
    else if (reg == 0x1B4u) code = 5;
    if ((int)st[2] + i < 25) code = 0;  // fewer than 26 bits of the stream so far
    if (L.bits) L.bits[(size_t)s * L.n_sym + i] = (uint8_t)bit;
    if (L.codes) L.codes[(size_t)s * L.n_sym + i] = (uint8_t)code;
}

// The carry for the next call, one workgroup a stream, after everything that reads the old one.
__global__ void __launch_bounds__(128) rdsb_state_kernel(RdsBitsLaunch L) {
    const int s = blockIdx.x, t = threadIdx.x;
    const float* m = L.mix + (size_t)s * L.mix_stride;
    uint8_t* st = L.state + (size_t)s * kRdsbStateBytes;
    // n_if >= 128 down > kRdsbHist and n_sym >= 76 > kRdsbTail: whole windows
    L.hist[(size_t)s * kRdsbHist + t] = m[L.n_if - kRdsbHist + t];
    if (t < kRdsbTail) st[4 + t] = L.sym[(size_t)s * L.n_sym + L.n_sym - kRdsbTail + t];
    if (t == 0) {
        st[0] = L.sign[(size_t)s * L.n_out + L.n_out - 1];
        st[1] = L.lastchip[(size_t)s * L.n_win + L.n_win - 1];
        st[2] = 25;  // n_sym >= 76 bits seen
    }
}

}  // namespace

int launch_rds_bits(const RdsBitsLaunch& L, int n_streams, hipStream_t s) {
    if (L.n_win <= 0 || n_streams <= 0) return 0;
    if (L.down <= 0 || L.down > kMaxDown || L.n_out != L.n_win * kRdsbWin || L.n_sym != L.n_win * kRdsbSyms ||
        (long long)L.n_out * L.down != (long long)L.n_if * kUp)
        return -1;
    hipLaunchKernelGGL(rdsb_resample_kernel, dim3(L.n_out / kChunkOut, n_streams), dim3(kResThreads), 0, s, L);
    hipLaunchKernelGGL(rdsb_phase_kernel, dim3(L.n_win, n_streams), dim3(256), 0, s, L);
    hipLaunchKernelGGL(rdsb_symbol_kernel, dim3(L.n_win, n_streams), dim3(128), 0, s, L);
    hipLaunchKernelGGL(rdsb_code_kernel, dim3((L.n_sym + 255) / 256, n_streams), dim3(256), 0, s, L);
    hipLaunchKernelGGL(rdsb_state_kernel, dim3(n_streams), dim3(kRdsbHist), 0, s, L);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace fmrx
