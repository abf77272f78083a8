// quiet.hip — quieting: every stream's treble rolled off (high-cut) and its audio turned
// down (soft mute) by the discriminator noise above the RDS skirt, per 64 ms meter frame, in front of
// de-emphasis and the S16 quantiser.  MONO and STEREO contexts alike.
//
// quiet_levels_kernel, one lane per (stream, frame f): from the meter's powers n = fl(power[61 kHz] +
// power[63 kHz]) of the frames f-3 .. f (the carry's where they lie in front of the call, 0 in front of the
// stream),
//
//   N = fl(fl(fl(n[f-3] + n[f-2]) + n[f-1]) + n[f]),  c = #{ j : N <= Tc[j] },  m = #{ j : N <= Tm[j] }
//
// two bytes a frame into a row of 2 (frames + 1) bytes whose pair 0 is the one carried in.  The thresholds
// are a `const __restrict__` kernel-argument pointer read at constant indices: scalar loads.  The carry is
// double-buffered: the lane of a stream's last frame writes the next call's into carry_out while a first
// lane may still read carry_in.
//
// quiet_apply_kernel, deemph_kernel's shape: a workgroup takes kQuietChunk outputs of one row (a stream's
// channel); their inputs and the 63 before them go to LDS once, each lane reads the 67 floats its four
// consecutive outputs need as 17 ds_read_b128 and keeps them in registers; the taps are scalar loads.  For
// audio frame n of the call, r = n / A, a = n mod A, u = a Gm, f = r Gm + u / A, t = u mod A,
// qc = c[f-1] (A - t) + c[f] t, qm the same over m.  With x the input and v its 64-tap FIR (acc = fl(acc +
// fl(h[k] x[n-k])) from 0, k ascending):
//
//   qc == 16 A: y = x bit for bit; elsewhere w = fl((float)(16 A - qc) cw), d = fl(v - x), e = fl(w d), y = fl(x + e)
//   qm == 16 A: z = y bit for bit; elsewhere g = fl(g0 + fl((float)qm cg)), z = fl(g y)
//
// The two divisions are paid once a lane; from there f and t step with 32-bit adds (t += Gm, a carry into f
// at A) and the level bytes are read again only when f moves.  A chunk touches at most three level pairs:
// where all of its cut levels are 16 every qc of it is 16 A and the workgroup skips the FIR (a
// workgroup-uniform branch; the definition makes it exact).  The row's last workgroup writes the next
// call's 63 inputs from its LDS image into state_out.  Not in place: neighbouring workgroups read each
// other's inputs as halo.  Built without FP contraction.
#include <hip/hip_runtime.h>

#include "dsp_device.h"
#include "fmrx_internal.h"

namespace fmrx {

namespace {

constexpr int kThreads = 256;
constexpr int kN61 = 5, kN63 = 6;                    // the tones of a frame's seven that the levels read
constexpr int kPer = kQuietChunk / kThreads;         // consecutive outputs a lane
constexpr int kImage = kQuietChunk + kQuietTaps;     // floats staged: 63 of history, the chunk, one of padding
static_assert(kPer == 4, "a lane's outputs start on a float4 of the LDS image");
static_assert(kQuietTaps % 4 == 0, "whole float4 reads");

__global__ void __launch_bounds__(kThreads) quiet_levels_kernel(LevelsLaunch L, const float* __restrict__ thr, int n_streams) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)n_streams * L.frames) return;
    const int s = (int)(i / L.frames), f = (int)(i - (long long)s * L.frames);
    const float* pw = L.power + (size_t)s * L.frames * kMeterTones;
    const float* cin = L.carry_in + (size_t)s * kQuietCarry;
    float n[4];  // frames f-3 .. f, oldest first
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int fr = f - 3 + k;
        if (fr >= 0) {
            const float* p = pw + (size_t)fr * kMeterTones;
            n[k] = p[kN61] + p[kN63];
        } else {  // fr = -3 .. -1: the carry's slots 0 .. 2
            n[k] = cin[fr + 3];
        }
    }
    const float N = ((n[0] + n[1]) + n[2]) + n[3];
    int c = 0, m = 0;
#pragma unroll
    for (int j = 0; j < kQuietSteps; j++) {
        c += N <= thr[j] ? 1 : 0;
        m += N <= thr[kQuietSteps + j] ? 1 : 0;
    }
    uint8_t* row = L.levels + (size_t)s * 2 * ((size_t)L.frames + 1);
    if (f == 0) {  // a caller's carry: anything outside 0 .. 16 counts as 0
        row[0] = cin[3] >= 0.0f && cin[3] <= (float)kQuietSteps ? (uint8_t)(int)cin[3] : (uint8_t)0;
        row[1] = cin[4] >= 0.0f && cin[4] <= (float)kQuietSteps ? (uint8_t)(int)cin[4] : (uint8_t)0;
    }
    row[2 + 2 * f] = (uint8_t)c;
    row[3 + 2 * f] = (uint8_t)m;
    if (f == L.frames - 1) {
        float4* o = reinterpret_cast<float4*>(L.carry_out + (size_t)s * kQuietCarry);
        o[0] = make_float4(n[1], n[2], n[3], (float)c);
        o[1] = make_float4((float)m, 0.0f, 0.0f, 0.0f);
    }
}

// the meter frame of audio frame n of a row
__device__ inline unsigned frame_of(unsigned n, unsigned A, unsigned Gm) {
    const unsigned r = n / A, a = n - r * A;
    return r * Gm + a * Gm / A;
}

__global__ void __launch_bounds__(kThreads) quiet_apply_kernel(QuietApplyLaunch L, const float* __restrict__ h, int row0, int vec) {
    __shared__ float4 X4[kImage / 4];  // X[i]: sample c0 - 63 + i of the row (0 past its end)
    float* X = reinterpret_cast<float*>(X4);
    const int tid = threadIdx.x;
    const int row = row0 + (int)blockIdx.y;
    const int s = row / L.nch, ch = row - s * L.nch;
    const unsigned c0 = blockIdx.x * (unsigned)kQuietChunk;
    const float* in = L.in + (size_t)s * L.stride + ch;
    const float* st = L.state_in + (size_t)row * kQuietHist;
    for (int i = tid; i < kImage; i += kThreads) {
        const long long g = (long long)c0 + i - kQuietHist;
        float v = 0.0f;
        if (g < 0) v = st[kQuietHist + g];  // only the first chunk: g >= -63
        else if (g < (long long)L.n) v = in[(size_t)g * L.nch];
        X[i] = v;
    }
    __syncthreads();
    const uint8_t* lv = L.levels + (size_t)s * L.level_stride;
    // the chunk's cut levels, the same for every lane: pairs fa .. fb + 1, at most three
    const unsigned last = L.n - c0 < (unsigned)kQuietChunk ? L.n - 1 : c0 + (unsigned)kQuietChunk - 1;
    const unsigned fa = frame_of(c0, L.A, L.Gm), fb = frame_of(last, L.A, L.Gm);
    bool open = true;
    for (unsigned e = fa; e <= fb + 1; e++) open = open && lv[2 * e] == kQuietSteps;
    const unsigned n0 = c0 + (unsigned)(kPer * tid);
    if (n0 < L.n) {
        // outputs 4 tid + r, r < 4: x[j] = X[4 tid + j], output r reads x[r + 63 - k] at tap k
        float acc[kPer] = {0.0f, 0.0f, 0.0f, 0.0f};
        float xin[kPer];
        if (open) {
            const float4 a = X4[tid + kQuietTaps / 4 - 1], b = X4[tid + kQuietTaps / 4];
            xin[0] = a.w, xin[1] = b.x, xin[2] = b.y, xin[3] = b.z;
        } else {
            float x[kQuietTaps + 4];
#pragma unroll
            for (int q = 0; q < kQuietTaps / 4 + 1; q++) {
                const float4 v = X4[tid + q];
                x[4 * q] = v.x;
                x[4 * q + 1] = v.y;
                x[4 * q + 2] = v.z;
                x[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int k = 0; k < kQuietTaps; k++) {
                const float hk = h[k];
#pragma unroll
                for (int r = 0; r < kPer; r++) {
                    const float p = hk * x[r + kQuietHist - k];
                    acc[r] = acc[r] + p;
                }
            }
#pragma unroll
            for (int r = 0; r < kPer; r++) xin[r] = x[r + kQuietHist];
        }
        const unsigned r0 = n0 / L.A, a0 = n0 - r0 * L.A, u = a0 * L.Gm;
        unsigned f = u / L.A, t = u - f * L.A;
        f += r0 * L.Gm;
        unsigned c0l = lv[2 * f], m0l = lv[2 * f + 1], c1l = lv[2 * f + 2], m1l = lv[2 * f + 3];
        const unsigned full = 16u * L.A;
        float z[kPer];
#pragma unroll
        for (int r = 0; r < kPer; r++) {
            const unsigned qc = c0l * (L.A - t) + c1l * t, qm = m0l * (L.A - t) + m1l * t;
            const float w = (float)(full - qc) * L.cw;
            const float d = acc[r] - xin[r];
            const float e = w * d;
            const float cut = xin[r] + e;
            const float y = qc == full ? xin[r] : cut;
            const float gq = (float)qm * L.cg;
            const float g = L.g0 + gq;
            const float muted = g * y;
            z[r] = qm == full ? y : muted;
            t += L.Gm;
            if (t >= L.A) {  // the next meter frame (at a granule's end too: u = A Gm there)
                t -= L.A;
                f++;
                c0l = c1l, m0l = m1l;
                if (n0 + (unsigned)r + 1 < L.n) c1l = lv[2 * f + 2], m1l = lv[2 * f + 3];  // nothing past the row's last pair is read
            }
        }
        const size_t at = (size_t)s * L.stride + ch + (size_t)n0 * L.nch;
        if (vec && n0 + kPer <= L.n) {  // nch == 1, the rows 16-byte (PCM: 8-byte) aligned
            if (L.out) *reinterpret_cast<float4*>(L.out + at) = make_float4(z[0], z[1], z[2], z[3]);
            if (L.pcm) {
                const uint32_t lo = (uint32_t)(uint16_t)quantize_s16(z[0]) | ((uint32_t)(uint16_t)quantize_s16(z[1]) << 16);
                const uint32_t hi = (uint32_t)(uint16_t)quantize_s16(z[2]) | ((uint32_t)(uint16_t)quantize_s16(z[3]) << 16);
                *reinterpret_cast<uint2*>(L.pcm + at) = make_uint2(lo, hi);
            }
        } else {
#pragma unroll
            for (int r = 0; r < kPer; r++) {
                if (n0 + (unsigned)r >= L.n) continue;
                const size_t o = at + (size_t)r * L.nch;
                if (L.out) L.out[o] = z[r];
                if (L.pcm) L.pcm[o] = quantize_s16(z[r]);
            }
        }
    }
    // the next call's history: the last 63 of (history ++ input), all inside the last chunk's image
    if (blockIdx.x == gridDim.x - 1 && tid < kQuietHist)
        L.state_out[(size_t)row * kQuietHist + tid] = X[(L.n - c0) + tid];
}

}  // namespace

int launch_quiet_levels(const LevelsLaunch& L, int n_streams, hipStream_t s) {
    if (n_streams <= 0) return 0;
    if (L.frames < 1 || L.carry_in == L.carry_out) return -1;
    const long long lanes = (long long)n_streams * L.frames;
    const long long blocks = (lanes + kThreads - 1) / kThreads;
    if (blocks > 0x7FFFFFFFll) return -1;
    hipLaunchKernelGGL(quiet_levels_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, L, L.thr, n_streams);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_quiet_apply(const QuietApplyLaunch& L, int n_streams, hipStream_t s) {
    if (L.n == 0 || n_streams <= 0) return 0;
    // q = l (A - t) + l' t <= 16 A converts to float exactly and u = a Gm < A Gm stays below 2^32
    // (Gm <= A: t steps into the next meter frame at most once an audio frame)
    if (L.A == 0 || L.Gm == 0 || L.A > (1u << 20) || L.Gm > 1024u || L.Gm > L.A || L.n > 0x7FFFFFF0u) return -1;
    if (L.nch < 1 || L.nch > 2 || L.state_in == L.state_out || L.in == L.out || (!L.out && !L.pcm)) return -1;
    const int vec = L.nch == 1 && L.stride % 4 == 0 && reinterpret_cast<uintptr_t>(L.out) % 16 == 0 &&
                            reinterpret_cast<uintptr_t>(L.pcm) % 8 == 0
                        ? 1
                        : 0;
    const unsigned chunks = (L.n + kQuietChunk - 1) / kQuietChunk;
    const int rows = n_streams * L.nch;
    for (int row0 = 0; row0 < rows; row0 += 65535) {  // grid.y holds stream x channel
        const int ny = rows - row0 < 65535 ? rows - row0 : 65535;
        hipLaunchKernelGGL(quiet_apply_kernel, dim3(chunks, (unsigned)ny), dim3(kThreads), 0, s, L, L.h, row0, vec);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace fmrx
