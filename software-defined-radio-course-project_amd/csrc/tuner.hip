// tuner.hip — the frequency-translating front end: raw I/Q -> rotate by a per-stream offset ->
// RF LPF + decimate -> FM demod, one launch, demod rows out (the audio stages of engine.cpp take them
// unchanged).  A stream tuned to +f Hz multiplies pair n by e^(-j 2 pi f n / rf_fs), so a station
// at +f of the capture lands on 0 Hz; several streams may read ONE capture (iq_stride = 0).
//
// Arithmetic (the contract the tests check bit for bit).  With g = gcd(|f|, rf_fs), N = rf_fs / g,
// k = (f / g) mod N and the table c[p] = (float)cos(2 pi p / N), s[p] = (float)sin(2 pi p / N)
// (double libm, rounded once), pair n -- the absolute pair index of the stream -- with the
// reference's normalised samples x_i, x_q (src/iofunc.cpp:67) and p = (k n) mod N becomes
//   I' = fl(fl(x_i c[p]) + fl(x_q s[p])),  Q' = fl(fl(x_q c[p]) - fl(x_i s[p]))
// and I', Q' then take the path x_i, x_q take in mono_fused.hip: resample (src/filter.cpp:67-103)
// as an ascending-tap sequential sum of separately rounded products, FMDemod (:106-133).
// The kernel rotates the integer samples u - 128 instead (x = (u - 128) 2^-7: every product and
// sum scales exactly, all values stay far from the subnormal range) and applies the 2^-7 once per
// RF output, in front of the discriminator.
// Input formats (TunerLaunch::format, fmrx.h FMRX_IQ_*): x = (u - 128) 2^-7 for u8, s 2^-7 for s8,
// s 2^-15 for little-endian s16, the float itself for f32 -- only the samples in front of the
// rotation differ.  The integer formats rotate the integers and scale once per RF output as above
// (nothing becomes subnormal); f32 takes no scale at all, so its arithmetic is the
// definition's operation for operation.  A lane's staging unit is two pairs in every format: a
// dword (u8, s8), a uint2 (s16), a float4 (f32).
//
// Decomposition: mono_fused.hip's.  A workgroup (one wave) walks a run of chunks of one stream;
// a pre-roll chunk in front rebuilds the RF history and the discriminator's previous I/Q from the
// raw bytes there (halo, then the call's bytes, then padding of the format's zero).  The phase of a
// pair is a function of its absolute index alone, so the pre-roll carries no rotator state: a workgroup
// reduces its first pair's index mod N in 64 bits once, then steps phases by conditional subtracts.
// Per chunk: coalesced unit loads (two pairs a lane, prefetched one chunk ahead), raw -> float,
// rotation against the stream's table (staged in LDS once per workgroup: N <= 4096 entries always
// fit), rotated pairs to LDS as float4; the RF FIR with I and Q together in packed f32 ops and the
// taps in VGPRs; the neighbour's last output by a DPP wave shift; demod to global memory.
// Every workgroup also moves a few words of the next call's halo (per stream, so a shared capture
// leaves each stream the same halo a private copy of the bytes would).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <numeric>

#include "dsp_device.h"
#include "iq_fmt.h"
#include "tuner.h"

namespace fmrx {

namespace {

constexpr int kNT = 64;      // one wave a workgroup
constexpr int kPreTail = 50; // demod samples of TunerLaunch::pre_tail (the audio FIR's history)

template <int T, int D, int R>
struct TunerCfg {
    static constexpr int NT = kNT;
    static constexpr int S = R * D;                     // pairs between adjacent threads
    static constexpr int G = (S % 4 == 2) ? 0 : 2;      // LDS pad pairs per S (bank spread)
    static constexpr int CIF = NT * R;                  // IF samples per chunk
    static constexpr int P = CIF * D;                   // I/Q pairs per chunk
    static constexpr int H = T - 1;                     // RF history pairs
    static constexpr int WH = T - 1 + D * (R - 1);      // highest window offset of a thread
    // LDS slot of buffer pair b (b = H + chunk-relative pair), mono_fused.hip's layout: pads of G
    // pairs every S pairs; (even b, b + 1) groups never straddle a pad
    static constexpr int slot(int b) { return b + G * (b / S); }
    static constexpr int XB = slot(H + P + 2) + 4;      // LDS pairs
    static constexpr int NLD = (P / 2) / NT;            // unit (2-pair) loads per thread and chunk
    static constexpr int LH0 = ((P - H) / 2) / NT;      // first load index holding history pairs
    static constexpr int NG = (T + 1) / 2;              // tap groups: {0}, {1,2}, {3,4}, ...
    static_assert(T % 2 == 1, "odd tap count");
    static_assert(S % 2 == 0 && H % 2 == 0, "pair groups must stay 16-B aligned");
    static_assert((P / 2) % NT == 0, "whole loads per chunk");
    static_assert(CIF >= kPreTail, "the pre-roll chunk holds the audio history");
};

template <int T, int D, int R, int PD, int F>
__global__ void __launch_bounds__(kNT) tuner_kernel(TunerLaunch L, MonoTaps taps) {
    using C = TunerCfg<T, D, R>;
    using Fmt = IqFmt<F>;
    using Raw = typename Fmt::Raw;
    constexpr int PB = Fmt::PB;                  // bytes an I/Q pair; a Raw holds two pairs
    constexpr int NT = kNT, CIF = C::CIF, P = C::P, H = C::H, S = C::S, G = C::G, NLD = C::NLD;
    constexpr int WH = C::WH, NG = C::NG;
    extern __shared__ float2 rot[];              // the stream's table: (c[p], s[p]), p < N
    __shared__ float4 xb4[C::XB / 2 + 1];        // rotated (I', Q') pairs scaled by 2^7, two per float4

    const int tid = threadIdx.x;
    const long long n_if = L.n_if;
    const int n_streams = (int)gridDim.x / L.segs;
    // the next call's halo: the last halo_bytes of halo ++ iq per stream, in dwords; nothing in
    // this launch reads halo_next
    {
        const size_t words = L.halo_bytes / 4, total = words * (size_t)n_streams;
        for (size_t i = (size_t)blockIdx.x * NT + tid; i < total; i += (size_t)gridDim.x * NT) {
            const size_t s = i / words, j = i - s * words, v = L.stream_bytes + 4 * j;  // into halo ++ iq
            const uint32_t w = v < L.halo_bytes
                                   ? *reinterpret_cast<const uint32_t*>(L.halo + s * L.halo_bytes + v)
                                   : *reinterpret_cast<const uint32_t*>(L.iq + s * L.iq_stride + (v - L.halo_bytes));
            *reinterpret_cast<uint32_t*>(L.halo_next + s * L.halo_bytes + 4 * j) = w;
        }
    }
    // chunk indices fit 32 bits for any HBM-resident stream; positions in the stream stay 64-bit
    const int n_chunks = (int)((n_if + CIF - 1) / CIF);
    const int stream = (int)blockIdx.x / L.segs;
    const int seg = (int)blockIdx.x - stream * L.segs;
    const int c0 = (int)((long long)seg * n_chunks / L.segs);
    const int c1 = (int)((long long)(seg + 1) * n_chunks / L.segs);
    if (c0 >= c1) return;
    const int c_full = (int)(L.stream_bytes / (PB * P));  // chunks lying wholly in the data

    const uint8_t* in = L.iq + (size_t)stream * L.iq_stride;
    const uint8_t* halo = L.halo + (size_t)stream * L.halo_bytes;
    const long long total = (long long)L.stream_bytes;
    const long long hb = (long long)L.halo_bytes;

    // ---- the stream's rotator: table to LDS, phases of this workgroup's first pairs
    const TunerStream ts = L.streams[stream];
    const uint32_t N = ts.N, k = ts.k;
    for (uint32_t i = tid; i < N; i += NT) rot[i] = L.tables[(size_t)ts.tab + i];
    const RotatorPhase rp(N, k, L.first_pair, (uint32_t)tid, (uint32_t)NT, (uint32_t)P);
    uint32_t pc = rp.of((long long)(c0 - 1) * P);  // phase of chunk c's first pair
    wave_sync();  // table staged

    // ---- prologue: RF history in front of the pre-roll chunk (pairs [(c0-1)P - H, (c0-1)P))
    for (int i = tid; i < H / 2; i += NT) {
        const long long rel = (long long)(c0 - 1) * P - H + 2 * i;
        const Raw w = load_unit<F>(in, halo, rel * PB, total, hb);
        const uint32_t p0 = rp.of(rel);
        xb4[C::slot(2 * i) / 2] = rotate2<F>(w, rot[p0], rot[addmod(p0, k, N)]);
    }
    // Input prefetch, one chunk ahead: always the same coalesced unit loads, from a base clamped
    // into the stream so that they never leave it; the chunks that touch the halo or run past the
    // end (c outside [0, c_full)) are rebuilt at staging time.
    Raw pf[NLD];
    auto fetch = [&](int cc) {
        if (c_full == 0) return;  // stream shorter than a chunk: every chunk is rebuilt
        const int cl = cc < 0 ? 0 : (cc < c_full ? cc : c_full - 1);
        const Raw* src = reinterpret_cast<const Raw*>(in + (size_t)cl * (PB * P)) + tid;
#pragma unroll
        for (int l = 0; l < NLD; l++) pf[l] = src[l * NT];
    };
    fetch(c0 - 1);

    float2 creg[NG];  // (c[2j-1], c[2j]); c[-1] = 0: straight from the kernel arguments
#pragma unroll
    for (int j = 0; j < NG; j++) creg[j] = make_float2(j == 0 ? 0.0f : taps.rf[2 * j - 1], taps.rf[2 * j]);
    float2v carry = {0.0f, 0.0f};  // last RF output of the previous chunk
    float4 hist[NLD - C::LH0];     // staged groups of the chunk's last H pairs (loads l >= LH0)
    for (int c = c0 - 1; c < c1; c++) {
        // ---- stage chunk c: lane u rotates pairs 2u, 2u + 1 and writes them as one float4
        if (!(c >= 0 && c < c_full)) {  // rare (one uniform branch): from the halo / padding
#pragma unroll
            for (int l = 0; l < NLD; l++)
                pf[l] = load_unit<F>(in, halo, (long long)c * (PB * P) + (long long)sizeof(Raw) * (tid + l * NT), total, hb);
        }
        uint32_t ph = addmod(pc, rp.tid, N);
#pragma unroll
        for (int l = 0; l < NLD; l++) {
            const int u = tid + l * NT;
            const float4 f = rotate2<F>(pf[l], rot[ph], rot[addmod(ph, k, N)]);
            ph = addmod(ph, rp.ld, N);
            xb4[C::slot(H + 2 * u) / 2] = f;
            if (l >= C::LH0) hist[l - C::LH0] = f;  // the chunk's last H pairs: next chunk's history
        }
        pc = addmod(pc, rp.chunk, N);
        wave_sync();  // (A) chunk c staged
        if (c + 1 < c1) fetch(c + 1);

        // ---- RF LPF + decimate (mono_fused.hip's loop): thread t owns outputs j = R t + r, r < R,
        // whose samples are window offsets o = D r + T-1-k (window base pair S t).  Tap-outer
        // order: each output is an ascending-k sequential sum while samples slide through a
        // register window.  Group 0 = tap 0, group j = taps 2j-1, 2j; loads run PD groups ahead.
#pragma unroll
        for (int j = 0; j < NG; j++) asm volatile("" : "+v"(creg[j]));  // opaque per chunk: no hoisted splats
        float2v acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = float2v{0.0f, 0.0f};
        float2v X[WH + 3];  // X[o] = window pair o, o in [0, WH+1]
        const float4* wb = xb4 + ((S + G) / 2) * tid;
        auto ld = [&](int o) {  // o even: pairs (o, o+1), one ds_read_b128
            const float4 q = wb[(o + G * (o / S)) / 2];
            X[o] = float2v{q.x, q.y};
            X[o + 1] = float2v{q.z, q.w};
        };
        auto ldg = [&](int j) {  // loads of group j
            if (j >= 1 && j < NG) ld(T - 1 - 2 * j);
        };
#pragma unroll
        for (int o = T - 1; o <= WH; o += 2) ld(o);
#pragma unroll
        for (int j = 0; j < PD; j++) ldg(j);
#pragma unroll
        for (int j = 0; j < NG; j++) {
            ldg(j + PD);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int kk = 2 * j - 1 + h;
                if (kk >= 0) {
                    const float ck = h == 0 ? creg[j].x : creg[j].y;
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const float2v p = X[T - 1 - kk + D * r] * ck;
                        acc[r] = acc[r] + p;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // pin the accumulators (the FIR chains stay in front of the hand-off), then the power of
        // two of the normalisation (2^-7, 2^-15; none for f32), exact, once per output
#pragma unroll
        for (int r = 0; r < R; r++) asm volatile("" ::"v"(acc[r]));
        if constexpr (F != kIqF32) {
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = acc[r] * Fmt::SCALE;
        }
        wave_sync();  // (B) all RF reads of xb done

        // ---- carries for chunk c+1: RF history (the chunk's pairs [P - H, P) -> [0, H)) from the
        // staging registers, last I/Q by a DPP wave shift (lane 0 keeps the previous chunk's)
#pragma unroll
        for (int l = C::LH0; l < NLD; l++) {
            const int i = tid + l * NT - (P - H) / 2;  // history group of staging lane u = tid + l NT
            if (i >= 0) xb4[C::slot(2 * i) / 2] = hist[l - C::LH0];
        }
        float2v prev;
        prev.x = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(carry.x), __float_as_int(acc[R - 1].x),
                                                            0x138, 0xF, 0xF, false));
        prev.y = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(carry.y), __float_as_int(acc[R - 1].y),
                                                            0x138, 0xF, 0xF, false));
        carry.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc[R - 1].x), NT - 1));
        carry.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc[R - 1].y), NT - 1));
        if (c >= c0 || (L.pre_tail && c == -1)) {
            float* out = L.demod + (size_t)stream * L.demod_stride + L.demod_hist;
            const long long g0 = (long long)c * CIF + R * tid;  // IF index of the lane's first output
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float2v pv = r == 0 ? prev : acc[r - 1];
                const float d = fm_demod_one(acc[r].x, acc[r].y, pv.x, pv.y);
                const long long g = g0 + r;
                if (g < n_if && g >= (c >= c0 ? 0 : -kPreTail)) out[g] = d;
            }
        }
    }
}

template <int T, int D, int R, int PD, int F>
int launch_format(const TunerLaunch& L, int n_streams, int max_n, const MonoTaps& taps, hipStream_t s) {
    hipLaunchKernelGGL((tuner_kernel<T, D, R, PD, F>), dim3(n_streams * L.segs), dim3(kNT),
                       sizeof(float2) * (size_t)max_n, s, L, taps);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <int T, int D, int R, int PD>
int launch_variant(const TunerLaunch& L, int n_streams, int max_n, const MonoTaps& taps, hipStream_t s) {
    switch (L.format) {
        case kIqU8: return launch_format<T, D, R, PD, kIqU8>(L, n_streams, max_n, taps, s);
        case kIqS8: return launch_format<T, D, R, PD, kIqS8>(L, n_streams, max_n, taps, s);
        case kIqS16: return launch_format<T, D, R, PD, kIqS16>(L, n_streams, max_n, taps, s);
        case kIqF32: return launch_format<T, D, R, PD, kIqF32>(L, n_streams, max_n, taps, s);
    }
    return -1;
}

// static LDS of a variant (the staged pairs) in bytes
int variant_lds(int rf_taps, int rf_decim) {
    const int r = rf_decim == 9 ? 2 : 3;
    const int pairs = (rf_taps - 1) + kNT * r * rf_decim;
    return 8 * (pairs + pairs / (r * rf_decim) * 2 + 8);
}

}  // namespace

bool tuner_design(int rf_fs, int offset_hz, int* N, int* k, float* cos_sin, int* why) {
    if (why) *why = 0;
    const long long f = offset_hz, a = f < 0 ? -f : f;
    if (rf_fs <= 0 || 2 * a >= (long long)rf_fs) {
        if (why) *why = 1;
        return false;
    }
    const long long g = std::gcd(a, (long long)rf_fs);  // gcd(0, rf_fs) = rf_fs: N = 1, k = 0
    const long long n = rf_fs / g;
    if (n > kTunerMaxN) {
        if (why) *why = 2;
        return false;
    }
    const long long kk = ((f / g) % n + n) % n;
    if (N) *N = (int)n;
    if (k) *k = (int)kk;
    if (cos_sin) {
        for (long long p = 0; p < n; p++) {  // the angle as (2 pi p) / N, one rounding each
            const double a = (2.0 * 3.14159265358979323846 * (double)p) / (double)n;
            cos_sin[2 * p] = (float)std::cos(a);
            cos_sin[2 * p + 1] = (float)std::sin(a);
        }
    }
    return true;
}

bool tuner_supported(int rf_taps, int rf_decim) {
    return (rf_taps == 51 || rf_taps == 101) && (rf_decim == 10 || rf_decim == 4 || rf_decim == 9);
}

int tuner_segments(long long n_if, int rf_taps, int rf_decim, int n_streams, int cus, int max_n) {
    const long long cif = (long long)kNT * (rf_decim == 9 ? 2 : 3);
    const long long chunks = (n_if + cif - 1) / cif;
    // resident workgroups a CU: 160 KiB of LDS, at most two waves a SIMD
    const int lds = variant_lds(rf_taps, rf_decim) + 8 * max_n;
    const long long target_wg = (long long)std::max(1, cus) * std::min(8, std::max(1, 160 * 1024 / lds));
    // mono_segments' rule: one wave of workgroups, segments of at least four chunks, and a call
    // too short to fill the grid even so takes one chunk a segment
    if ((long long)n_streams * chunks <= target_wg) return (int)std::max<long long>(1, chunks);
    long long segs = std::max<long long>(1, target_wg / std::max(1, n_streams));
    segs = std::min(segs, std::max<long long>(1, chunks / 4));
    return (int)segs;
}

int launch_tuner(const TunerLaunch& L, int n_streams, int rf_taps, int rf_decim, int max_n, const MonoTaps& taps,
                 hipStream_t s) {
    if (max_n < 1 || max_n > kTunerMaxN || L.segs < 1) return -1;
    if (rf_decim == 10 && rf_taps == 51) return launch_variant<51, 10, 3, 4>(L, n_streams, max_n, taps, s);
    if (rf_decim == 10 && rf_taps == 101) return launch_variant<101, 10, 3, 4>(L, n_streams, max_n, taps, s);
    if (rf_decim == 4 && rf_taps == 51) return launch_variant<51, 4, 3, 4>(L, n_streams, max_n, taps, s);
    if (rf_decim == 4 && rf_taps == 101) return launch_variant<101, 4, 3, 4>(L, n_streams, max_n, taps, s);
    // mode 3 (odd decimation 9): R = 2 keeps the per-thread stride S = 18 even
    if (rf_decim == 9 && rf_taps == 51) return launch_variant<51, 9, 2, 3>(L, n_streams, max_n, taps, s);
    if (rf_decim == 9 && rf_taps == 101) return launch_variant<101, 9, 2, 3>(L, n_streams, max_n, taps, s);
    return -1;
}

}  // namespace fmrx
