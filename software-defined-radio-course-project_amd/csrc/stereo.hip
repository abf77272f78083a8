// stereo.hip — the stereo half of the receive chain (src/project.cpp:152-193) around the pilot
// PLL (pll.hip): channel + carrier band-pass before it; after it the NCO pass over the PLL's
// trigArgs, the mixer, the audio LPF with the reference's SHARED audio_state, the mono delay line,
// L/R matrix and the R,L S16 quantiser.
//
// REF_EXACT semantics: in project.cpp the mono and stereo resample calls of
// one block share one history vector (project.cpp:114,146,172), so
//   * mono   of block b uses as history the last samples of block b-1's MIXER output;
//   * stereo of block b uses as history the last samples of block b's own DEMOD input.
// Both are reproduced exactly at the reference's block boundaries; this is the only
// place where the reference block size (SURVEY table M) changes the numbers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "dsp_device.h"
#include "fmrx_internal.h"
#include "pll_cr.h"
#include "pll_device.h"
#include "pll_math.h"

namespace fmrx {

namespace {

constexpr int kBpMax = 64;

struct BpTaps {
    float2 c[kBpMax];  // (channel, carrier) tap k, interleaved: one SGPR pair per packed product
};

// Channel (22-54 kHz) and carrier (18.5-19.5 kHz) band-pass FIRs share their input, so they
// run as ONE packed FIR: (acc_ch, acc_ca) += (h_ch[k], h_ca[k]) * x, two exact f32 lanes per
// v_pk op, each a sequential ascending-k sum (filter.cpp:84-92, up = down = 1).
template <int BT>
__global__ void __launch_bounds__(256) bpf_pair_kernel(StereoLaunch L, BpTaps t) {
    const int s = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= L.n_if) return;
    const float* x = L.demod + (size_t)s * L.demod_stride + L.hist + j;
    float2v acc = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < BT; k++) {
        const float xv = x[-k];
        const float2v p = float2v{t.c[k].x, t.c[k].y} * xv;
        acc = acc + p;
    }
    L.channel[(size_t)s * L.out_stride + j] = acc.x;
    L.carrier[(size_t)s * L.out_stride + j] = acc.y;
}

// The same FIR pair tiled through LDS: a workgroup stages kBpTile outputs' demod samples plus
// BT-1 of history once (coalesced), each thread keeps the window of its kBpR consecutive
// outputs in registers (one ds_read_b128 per 4 samples, lane stride 16 B: conflict-free) and
// the interleaved (h_ch, h_ca) taps are kernel arguments (SGPR pairs in the packed products).  Each output is
// still the ascending-k sequential sum of separately rounded products (filter.cpp:84-92).
// Replaces one global load per tap per output (51 VMEM instructions an output): 19.4 -> 15.1
// ms per call at 1,024 streams x 10 s.  Measured and dropped: workgroups walking 8 tiles with
// the next tile's loads in flight, and 8 outputs a thread (the taps then spill from SGPRs).
constexpr int kBpR = 4, kBpThreads = 256, kBpTile = kBpR * kBpThreads;  // (the pin below names 4)
template <int BT, bool SRC>
__global__ void __launch_bounds__(kBpThreads) bpf_pair_tile_kernel(StereoLaunch L, BpTaps t) {
    constexpr int W = kBpR + BT - 1;  // a thread's window: samples 4 tid .. 4 tid + W - 1 of the tile
    constexpr int WV = (W + 1) / 2;   // float4 reads (two duplicated samples each)
    // xs2[i] = (x, x), x = demod sample j0 - (BT - 1) + i: the packed product (h_ch, h_ca) * (x, x)
    // needs no splat; the L.hist >= BT - 1 history samples sit in front of the call's demod
    __shared__ float4 xs4[(kBpTile + BT - 1 + 1) / 2 + WV];
    float2* xs2 = reinterpret_cast<float2*>(xs4);
    const int s = blockIdx.y, tid = threadIdx.x;
    const long long j0 = (long long)blockIdx.x * kBpTile;
    const float* x = L.demod + (size_t)s * L.demod_stride + L.hist + j0 - (BT - 1);
    const long long avail = (long long)L.n_if - j0 + (BT - 1);  // samples of this stream from x on
    if constexpr (SRC) {  // the new samples from L.src (this tile's own ones also stored behind the history)
        // every load issued before any store (src may be host memory: one round trip, not one per
        // pass; src and demod could alias as far as the compiler knows)
        constexpr int kPass = (kBpTile + BT - 1 + kBpThreads - 1) / kBpThreads;
        const float* src = L.src + (size_t)s * L.n_if + j0 - (BT - 1);
        float* dst = const_cast<float*>(x);
        float v[kPass];
#pragma unroll
        for (int r = 0; r < kPass; r++) {
            const int i = tid + kBpThreads * r;
            const long long g = j0 - (BT - 1) + i;  // call index of sample i (< 0: history)
            v[r] = i < kBpTile + BT - 1 && i < avail ? (g < 0 ? x[i] : src[i]) : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < kPass; r++) {
            const int i = tid + kBpThreads * r;
            if (i >= kBpTile + BT - 1) break;
            if (i >= BT - 1 && i < avail) dst[i] = v[r];
            xs2[i] = make_float2(v[r], v[r]);
        }
    } else {
        for (int i = tid; i < kBpTile + BT - 1; i += kBpThreads) {
            const float v = i < avail ? x[i] : 0.0f;
            xs2[i] = make_float2(v, v);
        }
    }
    __syncthreads();
    float2v win[2 * WV];
#pragma unroll
    for (int q = 0; q < WV; q++) {  // lane stride 32 B
        const float4 w = xs4[2 * tid + q];
        win[2 * q] = float2v{w.x, w.y};
        win[2 * q + 1] = float2v{w.z, w.w};
    }
    float2v acc[kBpR];
#pragma unroll
    for (int r = 0; r < kBpR; r++) acc[r] = float2v{0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < BT; k++) {
        float2v pv[kBpR];  // the products first, then the sums: no sum reads the product just made
#pragma unroll
        for (int r = 0; r < kBpR; r++) pv[r] = float2v{t.c[k].x, t.c[k].y} * win[r + BT - 1 - k];  // output j0 + 4 tid + r, tap k
#pragma unroll
        for (int r = 0; r < kBpR; r++) acc[r] = acc[r] + pv[r];
        // tap-outer order kept (the accumulators pinned tap by tap, or LLVM sinks each output's
        // chain whole to its store): the kBpR chains interleave, so no packed result is read by
        // the next instruction (that costs a wait state on gfx950)
        asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
    }
    const long long j = j0 + (long long)kBpR * tid;
#pragma unroll
    for (int r = 0; r < kBpR; r++) {
        if (j + r < L.n_if) {
            L.channel[(size_t)s * L.out_stride + j + r] = acc[r].x;
            L.carrier[(size_t)s * L.out_stride + j + r] = acc[r].y;
        }
    }
}

__global__ void bpf_pair_generic(StereoLaunch L, BpTaps t) {
    const int s = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= L.n_if) return;
    const float* x = L.demod + (size_t)s * L.demod_stride + L.hist + j;
    float a = 0.0f, b = 0.0f;
    for (int k = 0; k < L.bp_taps; k++) {
        const float pa = t.c[k].x * x[-k];
        const float pb = t.c[k].y * x[-k];
        a = a + pa;
        b = b + pb;
    }
    L.channel[(size_t)s * L.out_stride + j] = a;
    L.carrier[(size_t)s * L.out_stride + j] = b;
}

// ---- the NCO pass ----------------------------------------------------------------------------
// The parallel tail of the PLL, here and not in pll.hip because stereo_audio_small_kernel below
// inlines the same arithmetic and shares its out-of-line fallback (sincos_lib, a copy per
// translation unit): with pll_nco_kernel and the fallback test hook in this file the compiler
// builds that copy, and the small kernel around it, exactly as measured (without a caller that
// reads the sine it drops half of sincos_lib and allocates the small kernel's registers anew).
// filter.cpp:170: ncoOut[i] = cos(trigArg * nocoScale + phaseAdjust), float arithmetic inside,
// double cos, float result; also the ncoOut_state carry (filter.cpp:173).
__global__ void pll_nco_kernel(float* io, int n, size_t stride, const float* args, size_t astride,
                               float nco_scale, float phase_adjust, float* st) {
    const int s = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* x = io + (size_t)s * stride;
    const float a = args[(size_t)s * astride + i] * nco_scale + phase_adjust;
    float cv;
#ifdef FMRX_AB_NCO_COS
    if (!fast_cos_f(a, &cv)) cv = sincos_lib(a).y;  // A/B: only the cosine certified
#else
    float sv;
    if (!fast_sincos_f(a, &sv, &cv)) cv = sincos_lib(a).y;
#endif
    x[i] = cv;
    if (i == n - 1) st[8 * (size_t)s + 4] = cv;
}

// Test hook (fmrx_test_pll_fallback): the PLL's out-of-line fallbacks on given arguments.
// kind 0: sincos_lib(a) -> out[2i] = sin, out[2i + 1] = cos; kind 1: atan2_lib(a = y, b = x);
// kind 2: the NCO's cos (pll_nco_kernel: fast_sincos_f, else the fallback).
__global__ void pll_fallback_test_kernel(int kind, const float* a, const float* b, size_t n, float* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (kind == 0) {
        const float2 r = sincos_lib(a[i]);
        out[2 * i] = r.x;
        out[2 * i + 1] = r.y;
    } else if (kind == 1) {
        out[i] = atan2_lib(a[i], b[i]);
    } else {
        float sv, cv;
        if (!fast_sincos_f(a[i], &sv, &cv)) cv = sincos_lib(a[i]).y;
        out[i] = cv;
    }
}

// ---- audio stage -------------------------------------------------------------------------
struct AudioView {
    const float* d;    // demod of block b (index 0 = first sample of block b)
    const float* ch;   // channel of block b
    const float* nco;  // nco of block b
};

__device__ inline float mixer_at(const AudioView& v, int i) { return 2.0f * (v.ch[i] * v.nco[i]); }

// mono of block b, frame m (project.cpp:146): history = previous block's mixer tail
// (or the carried tail for the first block of a call).
// Output m of the resampler: phase k0 = (m down) mod up, base input j0 = floor(m down / up);
// taps k = k0 + i up (i ascending = k ascending, filter.cpp:84-92) against input j0 - i: one
// division per output, none per tap.  The prototype stays in its own order: at tap step i the
// lanes of a wave read inside one up-wide window (coalesced), where a phase-major table would
// scatter them over up rows.
struct Phase {
    long long j0;
    const float* c;  // c[i * up] = coeff[k0 + i up]
    int cnt;
};
__device__ inline Phase phase_of(const AudioLaunch& L, int m) {
    const long long nd = (long long)m * L.down;
    Phase p;
    p.j0 = nd / L.up;
    const int k0 = (int)(nd - p.j0 * L.up);
    p.cnt = (L.at - k0 + L.up - 1) / L.up;
    p.c = L.audio_c + k0;
    return p;
}

__device__ inline float mono_at(const AudioLaunch& L, const AudioView& cur, const AudioView& prv,
                                bool has_prev, const float* tail, int tl, int m) {
    const Phase ph = phase_of(L, m);
    float acc = 0.0f;
    for (int i = 0; i < ph.cnt; i++) {
        const long long j = ph.j0 - i;
        float x;
        if (j >= 0) x = cur.d[j];
        else x = has_prev ? mixer_at(prv, L.if_per_block + (int)j) : tail[tl + j];
        const float p = ph.c[i * L.up] * x;
        acc = acc + p;
    }
    return acc;
}

// stereo of block b, frame m (project.cpp:172): history = the same block's demod tail.
__device__ inline float stereo_at(const AudioLaunch& L, const AudioView& cur, int m) {
    const Phase ph = phase_of(L, m);
    float acc = 0.0f;
    for (int i = 0; i < ph.cnt; i++) {
        const long long j = ph.j0 - i;
        const float x = j >= 0 ? mixer_at(cur, (int)j) : cur.d[L.if_per_block + j];
        const float p = ph.c[i * L.up] * x;
        acc = acc + p;
    }
    return acc;
}

__device__ inline AudioView view(const AudioLaunch& L, int s, int b) {
    const size_t nif = (size_t)L.n_blocks * L.if_per_block;
    AudioView v;
    v.d = L.demod + (size_t)s * L.demod_stride + L.hist + (size_t)b * L.if_per_block;
    v.ch = L.channel + (size_t)s * nif + (size_t)b * L.if_per_block;
    v.nco = L.nco + (size_t)s * nif + (size_t)b * L.if_per_block;
    return v;
}

constexpr int kTail = 64;  // mixer tail kept across calls (>= ceil((at-1)/up) + 1)

__global__ void stereo_audio_kernel(AudioLaunch L, int b0) {
    // grid.x = blocks x frame tiles (no 65,535 limit on the block count), grid.y = streams;
    // blocks b0, b0 + 1, ... of the call
    const int ft = (L.frames_per_block + (int)blockDim.x - 1) / (int)blockDim.x;
    const int s = blockIdx.y;
    const int bl = blockIdx.x / ft;
    const int b = b0 + bl;
    const int m = (blockIdx.x - bl * ft) * blockDim.x + threadIdx.x;
    if (m >= L.frames_per_block) return;
    const AudioView cur = view(L, s, b);
    const AudioView prv = b > 0 ? view(L, s, b - 1) : cur;
    const float* tail = L.mix_tail + (size_t)s * kTail;
    const float mono = mono_at(L, cur, prv, b > 0, tail, kTail, m);
    float shift;  // project.cpp:152-159, 5-sample delay line
    if (m >= kMonoDelay) {
        shift = mono_at(L, cur, prv, b > 0, tail, kTail, m - kMonoDelay);
    } else if (b > 0) {
        const AudioView pp = b > 1 ? view(L, s, b - 2) : prv;
        shift = mono_at(L, prv, pp, b > 1, tail, kTail, L.frames_per_block - kMonoDelay + m);
    } else {
        shift = L.mono_state[(size_t)s * 8 + m];
    }
    const float st = stereo_at(L, cur, m);
    const float left = half_of(shift + st);    // filter.cpp:196
    const float right = half_of(shift - st);   // filter.cpp:197
    const size_t o = ((size_t)s * L.n_blocks + b) * (size_t)L.frames_per_block + m;
    L.pcm[2 * o] = quantize_s16(right);        // project.cpp:184-187 (R first)
    L.pcm[2 * o + 1] = quantize_s16(left);
    if (L.mono_out) L.mono_out[o] = mono;
    if (L.lr_out) L.lr_out[o] = make_float2(right, left);
}

// Modes 0/1 (up = 1): one workgroup per (block, stream).  The block's (demod, mixer) pairs sit in
// LDS behind the histories of both resamplers -- (previous block's mixer, own demod tail), the
// shared-audio_state quirk of project.cpp:146/172 -- so the mono and stereo LPF of a frame are
// ONE packed FIR over one float2 array (v_pk_mul/v_pk_add, each lane an ascending-tap
// sequential sum as filter.cpp:84-92), and the mono of each frame is computed once: the 5-frame
// delay line reads it back from LDS.  Same arithmetic as stereo_audio_kernel.
constexpr int kTileIf = 1024, kTileFrames = 256, kTileTaps = 64;

// carry (the small kernel's last block): the state carry from this tile's LDS instead of
// audio_state_carry's global re-reads -- MO holds the block's monos (mono_at's sums, same
// order) and X[H + i].y its mixer samples.
__device__ void audio_tile(const AudioLaunch& L, int s, int b, bool carry = false) {
    constexpr int kPer = kTileFrames / 128;    // frames per thread
    __shared__ float2 X[kTileTaps + kTileIf];  // X[H + j]: (mono input, stereo input) at IF index j
    __shared__ float C[kTileTaps], MO[kTileFrames];
    const int ipb = L.if_per_block, fpb = L.frames_per_block, at = L.at, H = at - 1;
    const AudioView cur = view(L, s, b);
    for (int i = threadIdx.x; i < ipb; i += blockDim.x) X[H + i] = make_float2(cur.d[i], mixer_at(cur, i));
    if (b > 0) {
        const AudioView prv = view(L, s, b - 1);
        for (int i = threadIdx.x; i < H; i += blockDim.x)
            X[i] = make_float2(mixer_at(prv, ipb - H + i), cur.d[ipb - H + i]);
    } else {
        for (int i = threadIdx.x; i < H; i += blockDim.x)
            X[i] = make_float2(L.mix_tail[(size_t)s * kTail + kTail - H + i], cur.d[ipb - H + i]);
    }
    for (int i = threadIdx.x; i < at; i += blockDim.x) C[i] = L.audio_c[i];
    __syncthreads();
    float st[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int m = threadIdx.x + 128 * k;
        st[k] = 0.0f;
        if (m < fpb) {
            const float2* x = X + H + m * L.down;
            float2v acc = {0.0f, 0.0f};
            for (int i = 0; i < at; i++) {
                const float2 v = x[-i];
                const float2v p = float2v{v.x, v.y} * C[i];
                acc = acc + p;
            }
            MO[m] = acc.x;
            st[k] = acc.y;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int m = threadIdx.x + 128 * k;
        if (m >= fpb) continue;
        float shift;  // project.cpp:152-159, 5-sample delay line
        if (m >= kMonoDelay) {
            shift = MO[m - kMonoDelay];
        } else if (b > 0) {  // the previous block's last frames read only its own demod (host-checked)
            const float* d = view(L, s, b - 1).d + (fpb - kMonoDelay + m) * L.down;
            float a = 0.0f;
            for (int i = 0; i < at; i++) {
                const float p = C[i] * d[-i];
                a = a + p;
            }
            shift = a;
        } else {
            shift = L.mono_state[(size_t)s * 8 + m];
        }
        const float left = half_of(shift + st[k]);   // filter.cpp:196
        const float right = half_of(shift - st[k]);  // filter.cpp:197
        const size_t o = ((size_t)s * L.n_blocks + b) * (size_t)fpb + m;
        L.pcm[2 * o] = quantize_s16(right);          // project.cpp:184-187 (R first)
        L.pcm[2 * o + 1] = quantize_s16(left);
        if (L.mono_out) L.mono_out[o] = MO[m];
        if (L.lr_out) L.lr_out[o] = make_float2(right, left);
    }
    if (!carry) return;
    __syncthreads();  // every read of the old mono_state / mix_tail happened above
    const int i = threadIdx.x;
    if (i < kMonoDelay) L.mono_state[(size_t)s * 8 + i] = MO[fpb - kMonoDelay + i];
    if (i < kTail) L.mix_tail[(size_t)s * kTail + i] = X[H + ipb - kTail + i].y;
}

__global__ void __launch_bounds__(128) stereo_audio_tile_kernel(AudioLaunch L, int b0) {
    audio_tile(L, blockIdx.y, b0 + (int)blockIdx.x);  // block b of the call, stream blockIdx.y
}

// Carry the audio state of the LAST block of this call into the next call (thread i of stream s).
__device__ void audio_state_carry(const AudioLaunch& L, int s, int i) {
    const int b = L.n_blocks - 1;
    const AudioView cur = view(L, s, b);
    const AudioView prv = b > 0 ? view(L, s, b - 1) : cur;
    const float* tail = L.mix_tail + (size_t)s * kTail;
    float mono = 0.0f, mix = 0.0f;
    if (i < kMonoDelay)
        mono = mono_at(L, cur, prv, b > 0, tail, kTail, L.frames_per_block - kMonoDelay + i);
    if (i < kTail) mix = mixer_at(cur, L.if_per_block - kTail + i);
    __syncthreads();  // every read of the old tail happens before it is overwritten
    if (i < kMonoDelay) L.mono_state[(size_t)s * 8 + i] = mono;
    if (i < kTail) L.mix_tail[(size_t)s * kTail + i] = mix;
}

__global__ void stereo_state_kernel(AudioLaunch L) { audio_state_carry(L, blockIdx.x, threadIdx.x); }

// A few blocks a stream (the reference's per-block seam, fmrx_audio_block with one block): the
// NCO (pll_nco_kernel's arithmetic, from the PLL's trigArgs), every block's audio in order
// (audio_tile), the state carry (stereo_state_kernel) and the demod history for the next call
// (the last kDemodHist samples to the front) in ONE launch, one workgroup a stream -- four
// launches fewer than the parallel path, which costs each of them ~4-7 us at this size
// (profiles/r06/seam: kernel trace of the seam).
__global__ void __launch_bounds__(128) stereo_audio_small_kernel(AudioLaunch L, const float* args, size_t astride,
                                                                 float nco_scale, float phase_adjust, float* pll_st,
                                                                 int demod_hist) {
    const int s = blockIdx.x;
    const int nif = L.n_blocks * L.if_per_block;
    float* nco = const_cast<float*>(L.nco) + (size_t)s * nif;
    for (int i = threadIdx.x; i < nif; i += blockDim.x) {  // filter.cpp:170 (pll_nco_kernel)
        const float a = args[(size_t)s * astride + i] * nco_scale + phase_adjust;
        float sv, cv;
        if (!fast_sincos_f(a, &sv, &cv)) cv = sincos_lib(a).y;
        nco[i] = cv;
        if (i == nif - 1) pll_st[8 * (size_t)s + 4] = cv;
    }
    __syncthreads();
    for (int b = 0; b < L.n_blocks; b++) {
        audio_tile(L, s, b, b == L.n_blocks - 1);  // the last block carries the state
        __syncthreads();
    }
    float* d = const_cast<float*>(L.demod) + (size_t)s * L.demod_stride;
    for (int i = threadIdx.x; i < demod_hist; i += blockDim.x) d[i] = d[nif + i];
}

inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -2; }

}  // namespace

int launch_bpf_pair(const StereoLaunch& L, int n_streams, hipStream_t s, bool tiled) {
    if (L.n_if <= 0) return 0;
    if (L.bp_taps > kBpMax) return -1;
    BpTaps t{};
    for (int k = 0; k < L.bp_taps; k++) t.c[k] = make_float2(L.ch_c[k], L.ca_c[k]);
    const dim3 grid((L.n_if + 255) / 256, n_streams), block(256);
    const bool tile = L.bp_taps == 51 && L.hist >= 50 && tiled;
    if (L.src && !tile &&  // the per-output kernels read the new samples from demod: copy them there
        hipMemcpy2DAsync(const_cast<float*>(L.demod) + L.hist, L.demod_stride * sizeof(float), L.src,
                         (size_t)L.n_if * sizeof(float), (size_t)L.n_if * sizeof(float), n_streams,
                         hipMemcpyDefault, s) != hipSuccess)
        return -1;
    if (tile && L.src)
        hipLaunchKernelGGL((bpf_pair_tile_kernel<51, true>), dim3((L.n_if + kBpTile - 1) / kBpTile, n_streams),
                           dim3(kBpThreads), 0, s, L, t);
    else if (tile)
        hipLaunchKernelGGL((bpf_pair_tile_kernel<51, false>), dim3((L.n_if + kBpTile - 1) / kBpTile, n_streams),
                           dim3(kBpThreads), 0, s, L, t);
    else if (L.bp_taps == 51)
        hipLaunchKernelGGL(bpf_pair_kernel<51>, grid, block, 0, s, L, t);
    else
        hipLaunchKernelGGL(bpf_pair_generic, grid, block, 0, s, L, t);
    return ok();
}

void launch_nco_pass(float* io, int n, int n_streams, size_t stride, const float* args, size_t astride,
                     const PllLoop& loop, float* st, hipStream_t s) {
    hipLaunchKernelGGL(pll_nco_kernel, dim3((n + 255) / 256, n_streams), dim3(256), 0, s, io, n, stride, args, astride,
                       loop.nco_scale, loop.phase_adjust, st);
}

int launch_stereo_audio_range(const AudioLaunch& L, int b0, int b1, bool last, int n_streams, hipStream_t s) {
    if (L.n_blocks <= 0 || b0 < 0 || b1 > L.n_blocks || b0 > b1) return 0;
    const int H = L.at - 1;
    if (b1 > b0) {
        if (L.up == 1 && L.if_per_block <= kTileIf && L.frames_per_block <= kTileFrames && L.at <= kTileTaps &&
            L.frames_per_block * L.down <= L.if_per_block && (L.frames_per_block - kMonoDelay) * L.down >= H) {
            hipLaunchKernelGGL(stereo_audio_tile_kernel, dim3(b1 - b0, n_streams), dim3(128), 0, s, L, b0);
        } else {
            const dim3 grid(((L.frames_per_block + 127) / 128) * (b1 - b0), n_streams);
            hipLaunchKernelGGL(stereo_audio_kernel, grid, dim3(128), 0, s, L, b0);
        }
    }
    if (last) hipLaunchKernelGGL(stereo_state_kernel, dim3(n_streams), dim3(kTail), 0, s, L);
    return ok();
}

int launch_stereo_audio_small(const AudioLaunch& L, int n_streams, const float* args, size_t astride, float nco_scale,
                              float phase_adjust, float* pll_st, int demod_hist, hipStream_t s) {
    if (L.up != 1 || L.if_per_block > kTileIf || L.frames_per_block > kTileFrames || L.at > kTileTaps ||
        L.if_per_block < kTail || L.n_blocks < 1 || demod_hist > L.n_blocks * L.if_per_block)
        return -1;
    hipLaunchKernelGGL(stereo_audio_small_kernel, dim3(n_streams), dim3(128), 0, s, L, args, astride, nco_scale,
                       phase_adjust, pll_st, demod_hist);
    return ok();
}

int launch_stereo_audio(const AudioLaunch& L, int n_streams, hipStream_t s) {
    return launch_stereo_audio_range(L, 0, L.n_blocks, true, n_streams, s);
}

int launch_pll_fallback_test(int kind, const float* a, const float* b, size_t n, float* out, hipStream_t s) {
    if (n == 0) return 0;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(pll_fallback_test_kernel, dim3(grid), dim3(256), 0, s, kind, a, b, n, out);
    return hipGetLastError() != hipSuccess;
}

}  // namespace fmrx
