// blend.hip — soft stereo: every stereo stream blended toward mono by the signal-to-noise
// ratio of its pilot, per 64 ms meter frame, in front of the S16 quantiser.  Two pointwise kernels, no LDS.
//
// blend_levels_kernel, one lane per (stream, frame f): from the meter's powers a = power[19 kHz],
// g = fl(power[17 kHz] + power[21 kHz]) of the frames f-3 .. f (the carry's where they lie in front of the
// call, 0 in front of the stream),
//
//   S = fl(fl(fl(a[f-3] + a[f-2]) + a[f-1]) + a[f]),  G the same over g,  level = #{ j : S >= fl(T[j] G) }
//
// one byte a frame into a row of frames + 1 bytes whose entry 0 is the level carried in.  The thresholds
// are a `const __restrict__` kernel-argument pointer read at constant indices: scalar loads.  The carry is
// double-buffered: the lane of a stream's last frame writes the next call's into carry_out while a first
// lane may still read carry_in.
//
// blend_apply_kernel, one lane per kBlendPer consecutive (right, left) frames of a row: for audio frame n
// of the call, r = n / A, a = n mod A, u = a Gm, f = r Gm + u / A, t = u mod A, q = l[f-1] (A - t) + l[f] t,
// k = fl((float)(16 A - q) c).  q == 16 A: the pair passes bit for bit.  Elsewhere d = fl(L - R),
// e = fl(k d), L' = fl(L - e), R' = fl(R + e).  The two divisions are paid once a lane; from there f and t
// step with 32-bit adds (t += Gm, a carry into f at A).  The input is two 16-byte loads, the floats go out
// as two 16-byte stores, the PCM of a frame as one 4-byte word (all four of a lane as one 16-byte store
// where the row allows it).  Built without FP contraction.
#include <hip/hip_runtime.h>

#include "dsp_device.h"
#include "fmrx_internal.h"

namespace fmrx {

namespace {

constexpr int kThreads = 256;
constexpr int kA = 1, kG17 = 0, kG21 = 2;  // the tones of a frame's seven that the levels read
static_assert(kBlendPer == 4, "a lane's frames are two float4 and its PCM one uint4");

__global__ void __launch_bounds__(kThreads) blend_levels_kernel(LevelsLaunch L, const float* __restrict__ thr, int n_streams) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)n_streams * L.frames) return;
    const int s = (int)(i / L.frames), f = (int)(i - (long long)s * L.frames);
    const float* pw = L.power + (size_t)s * L.frames * kMeterTones;
    const float* cin = L.carry_in + (size_t)s * kBlendCarry;
    float a[4], g[4];  // frames f-3 .. f, oldest first
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int fr = f - 3 + k;
        if (fr >= 0) {
            const float* p = pw + (size_t)fr * kMeterTones;
            a[k] = p[kA];
            g[k] = p[kG17] + p[kG21];
        } else {  // fr = -3 .. -1: the carry's slots 0 .. 2 (a) and 3 .. 5 (g)
            a[k] = cin[fr + 3];
            g[k] = cin[fr + 6];
        }
    }
    const float S = ((a[0] + a[1]) + a[2]) + a[3];
    const float G = ((g[0] + g[1]) + g[2]) + g[3];
    int level = 0;
#pragma unroll
    for (int j = 0; j < kBlendSteps; j++) level += S >= thr[j] * G ? 1 : 0;
    uint8_t* row = L.levels + (size_t)s * ((size_t)L.frames + 1);
    if (f == 0) row[0] = cin[6] >= 0.0f && cin[6] <= (float)kBlendSteps ? (uint8_t)(int)cin[6] : (uint8_t)0;  // a caller's carry
    row[1 + f] = (uint8_t)level;
    if (f == L.frames - 1) {
        float4* o = reinterpret_cast<float4*>(L.carry_out + (size_t)s * kBlendCarry);
        o[0] = make_float4(a[1], a[2], a[3], g[1]);
        o[1] = make_float4(g[2], g[3], (float)level, 0.0f);
    }
}

struct Mix {
    float r, l;
};

// one frame: the pair, the levels either side of its meter frame, its place t in it
__device__ inline Mix blend_one(float R, float Lf, unsigned l0, unsigned l1, unsigned t, unsigned A, float c, bool* pass) {
    const unsigned q = l0 * (A - t) + l1 * t;
    *pass = q == 16u * A;
    const float k = (float)(16u * A - q) * c;
    const float d = Lf - R;
    const float e = k * d;
    Mix m;
    m.l = Lf - e;
    m.r = R + e;
    return m;
}

__device__ inline uint32_t pcm_word(float R, float Lf) {
    return (uint32_t)(uint16_t)quantize_s16(R) | ((uint32_t)(uint16_t)quantize_s16(Lf) << 16);
}

__global__ void __launch_bounds__(kThreads) blend_apply_kernel(BlendApplyLaunch L, int row0, int pcm16) {
    const unsigned n0 = (blockIdx.x * kThreads + threadIdx.x) * kBlendPer;
    if (n0 >= L.n) return;
    const size_t s = (size_t)row0 + blockIdx.y;
    const uint8_t* lv = L.levels + s * L.level_stride;
    const float2* in = L.in + s * L.n + n0;
    const unsigned r = n0 / L.A, a = n0 - r * L.A, u = a * L.Gm;
    unsigned f = u / L.A, t = u - f * L.A;
    f += r * L.Gm;
    unsigned l0 = lv[f], l1 = lv[f + 1];
    const unsigned cnt = L.n - n0 < (unsigned)kBlendPer ? L.n - n0 : (unsigned)kBlendPer;
    float x[2 * kBlendPer];
    if (cnt == kBlendPer) {
        const float4 v0 = reinterpret_cast<const float4*>(in)[0], v1 = reinterpret_cast<const float4*>(in)[1];
        x[0] = v0.x, x[1] = v0.y, x[2] = v0.z, x[3] = v0.w;
        x[4] = v1.x, x[5] = v1.y, x[6] = v1.z, x[7] = v1.w;
    } else {
        for (unsigned i = 0; i < (unsigned)kBlendPer; i++) {
            const float2 v = i < cnt ? in[i] : make_float2(0.0f, 0.0f);
            x[2 * i] = v.x, x[2 * i + 1] = v.y;
        }
    }
#pragma unroll
    for (int i = 0; i < kBlendPer; i++) {
        bool pass;
        const Mix m = blend_one(x[2 * i], x[2 * i + 1], l0, l1, t, L.A, L.c, &pass);
        if (!pass) x[2 * i] = m.r, x[2 * i + 1] = m.l;
        t += L.Gm;
        if (t >= L.A) {  // the next meter frame (at a granule's end too: u = A Gm there)
            t -= L.A;
            f++;
            l0 = l1;
            l1 = (unsigned)i + 1 < cnt ? lv[f + 1] : l1;  // nothing past the row's last frame is read
        }
    }
    if (cnt == kBlendPer) {
        if (L.out) {
            float4* o = reinterpret_cast<float4*>(L.out + s * L.n + n0);
            o[0] = make_float4(x[0], x[1], x[2], x[3]);
            o[1] = make_float4(x[4], x[5], x[6], x[7]);
        }
        if (L.pcm) {
            uint32_t* p = reinterpret_cast<uint32_t*>(L.pcm) + s * L.n + n0;
            const uint4 w = make_uint4(pcm_word(x[0], x[1]), pcm_word(x[2], x[3]), pcm_word(x[4], x[5]), pcm_word(x[6], x[7]));
            if (pcm16) *reinterpret_cast<uint4*>(p) = w;
            else p[0] = w.x, p[1] = w.y, p[2] = w.z, p[3] = w.w;
        }
    } else {
        for (unsigned i = 0; i < cnt; i++) {
            if (L.out) L.out[s * L.n + n0 + i] = make_float2(x[2 * i], x[2 * i + 1]);
            if (L.pcm) reinterpret_cast<uint32_t*>(L.pcm)[s * L.n + n0 + i] = pcm_word(x[2 * i], x[2 * i + 1]);
        }
    }
}

}  // namespace

int launch_blend_levels(const LevelsLaunch& L, int n_streams, hipStream_t s) {
    if (n_streams <= 0) return 0;
    if (L.frames < 1 || L.carry_in == L.carry_out) return -1;
    const long long lanes = (long long)n_streams * L.frames;
    const long long blocks = (lanes + kThreads - 1) / kThreads;
    if (blocks > 0x7FFFFFFFll) return -1;
    hipLaunchKernelGGL(blend_levels_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, L, L.thr, n_streams);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_blend_apply(const BlendApplyLaunch& L, int n_streams, hipStream_t s) {
    if (L.n == 0 || n_streams <= 0) return 0;
    // q = l (A - t) + l' t <= 16 A and u = a Gm < A Gm stay below 2^24 and 2^32; the rows 16-byte aligned
    if (L.A == 0 || L.Gm == 0 || L.A > (1u << 20) || L.Gm > 1024u || L.n > 0x7FFFFFF0u || L.n % 2 != 0) return -1;
    if (reinterpret_cast<uintptr_t>(L.in) % 16 != 0 || reinterpret_cast<uintptr_t>(L.out) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(L.pcm) % 4 != 0)
        return -1;
    const int pcm16 = reinterpret_cast<uintptr_t>(L.pcm) % 16 == 0 && L.n % 4 == 0 ? 1 : 0;
    const unsigned blocks = (L.n + kThreads * kBlendPer - 1) / (kThreads * kBlendPer);
    for (int row0 = 0; row0 < n_streams; row0 += 65535) {  // grid.y holds the streams
        const int ny = n_streams - row0 < 65535 ? n_streams - row0 : 65535;
        hipLaunchKernelGGL(blend_apply_kernel, dim3(blocks, (unsigned)ny), dim3(kThreads), 0, s, L, row0, pcm16);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace fmrx
