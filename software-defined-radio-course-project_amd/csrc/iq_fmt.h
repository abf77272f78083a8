// iq_fmt.h — device helpers shared by the kernels that read raw I/Q (tuner.hip, wide.hip, rate.hip): the
// formats' two-pair staging unit, the unit load from a virtual stream (halo ++ data ++ zeros), the
// rotation of a unit against a (cos, sin) table, the rotator's phase steps and the single-wave LDS
// hand-off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsp_device.h"
#include "tuner.h"

namespace fmrx {

// u - 128 of byte K of w as an exact float
template <int K>
__device__ inline float sbyte(uint32_t w) {
    return static_cast<float>((w >> (8 * K)) & 0xFFu) - 128.0f;
}

// A raw format's staging unit: two I/Q pairs as one load (Raw), the unit of zeros (padding past the
// end of the stream), the samples as exact floats times 2^SH (the kernel rotates and filters these
// and applies SCALE = 2^-SH once per RF output; F32 takes the floats themselves, no scale).
template <int F>
struct IqFmt;
template <>
struct IqFmt<kIqU8> {
    using Raw = uint32_t;
    static constexpr int PB = 2;
    static constexpr float SCALE = 0.0078125f;
    static __device__ inline Raw zero() { return 0x80808080u; }
    static __device__ inline void unpack(Raw w, float2v& x0, float2v& x1) {
        x0 = float2v{sbyte<0>(w), sbyte<1>(w)};
        x1 = float2v{sbyte<2>(w), sbyte<3>(w)};
    }
};
template <>
struct IqFmt<kIqS8> {  // s = (s ^ 0x80 as u8) - 128: one xor a unit, then U8's conversion
    using Raw = uint32_t;
    static constexpr int PB = 2;
    static constexpr float SCALE = 0.0078125f;
    static __device__ inline Raw zero() { return 0u; }
    static __device__ inline void unpack(Raw w, float2v& x0, float2v& x1) {
        IqFmt<kIqU8>::unpack(w ^ 0x80808080u, x0, x1);
    }
};
template <>
struct IqFmt<kIqS16> {  // little-endian int16: I in the low half of a dword, Q in the high half
    using Raw = uint2;
    static constexpr int PB = 4;
    static constexpr float SCALE = 0.000030517578125f;  // 2^-15
    static __device__ inline Raw zero() { return make_uint2(0u, 0u); }
    static __device__ inline float lo(uint32_t w) { return static_cast<float>(static_cast<int>(w << 16) >> 16); }
    static __device__ inline float hi(uint32_t w) { return static_cast<float>(static_cast<int>(w) >> 16); }
    static __device__ inline void unpack(Raw w, float2v& x0, float2v& x1) {
        x0 = float2v{lo(w.x), hi(w.x)};
        x1 = float2v{lo(w.y), hi(w.y)};
    }
};
template <>
struct IqFmt<kIqF32> {
    using Raw = float4;
    static constexpr int PB = 8;  // no SCALE: the floats are the samples
    static __device__ inline Raw zero() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    static __device__ inline void unpack(Raw w, float2v& x0, float2v& x1) {
        x0 = float2v{w.x, w.y};
        x1 = float2v{w.z, w.w};
    }
};

// One unit (two I/Q pairs) of the virtual stream (halo ++ data ++ padding of the format's zero) at
// byte offset `off` (a multiple of the unit).  Pairs past the end read as x = 0.0.
template <int F>
__device__ inline typename IqFmt<F>::Raw load_unit(const uint8_t* in, const uint8_t* halo, long long off,
                                                   long long total, long long halo_bytes) {
    using Raw = typename IqFmt<F>::Raw;
    if (off >= 0) {
        if (off + (long long)sizeof(Raw) <= total) return *reinterpret_cast<const Raw*>(in + off);
        return IqFmt<F>::zero();
    }
    return *reinterpret_cast<const Raw*>(halo + (halo_bytes + off));
}
// The same of a stream that may be read further back than its halo (zeros ++ halo ++ data ++ zeros)
template <int F>
__device__ inline typename IqFmt<F>::Raw load_unit_bounded(const uint8_t* in, const uint8_t* halo, long long off,
                                                           long long total, long long halo_bytes) {
    using Raw = typename IqFmt<F>::Raw;
    if (off >= 0) {
        if (off + (long long)sizeof(Raw) <= total) return *reinterpret_cast<const Raw*>(in + off);
        return IqFmt<F>::zero();
    }
    if (off >= -halo_bytes) return *reinterpret_cast<const Raw*>(halo + (halo_bytes + off));
    return IqFmt<F>::zero();
}

// The two pairs x0, x1 rotated by table entries a (first pair) and b: (I', Q', I', Q'), every
// product and sum rounded separately (no FMA: -ffp-contract=off).
__device__ inline float4 rotate_pairs(float2v x0, float2v x1, float2 a, float2 b) {
    const float2v c0 = x0 * a.x, c1 = x1 * b.x;                        // (i c, q c)
    const float2v s0 = float2v{x0.y, -x0.x} * a.y, s1 = float2v{x1.y, -x1.x} * b.y;  // (q s, -(i s))
    const float2v r0 = c0 + s0, r1 = c1 + s1;
    return make_float4(r0.x, r0.y, r1.x, r1.y);
}
template <int F>
__device__ inline float4 rotate2(typename IqFmt<F>::Raw w, float2 a, float2 b) {
    float2v x0, x1;
    IqFmt<F>::unpack(w, x0, x1);
    return rotate_pairs(x0, x1, a, b);
}
// The same with the integer formats normalised first (x = integer 2^-7 / 2^-15: exact): what the
// capture stage's kernels stage, whose rows hold the samples themselves
template <int F>
__device__ inline float4 rotate_scaled(typename IqFmt<F>::Raw w, float2 a, float2 b) {
    float2v x0, x1;
    IqFmt<F>::unpack(w, x0, x1);
    if constexpr (F != kIqF32) {
        x0 = x0 * IqFmt<F>::SCALE;
        x1 = x1 * IqFmt<F>::SCALE;
    }
    return rotate_pairs(x0, x1, a, b);
}

// a + b mod n for a, b < n
__device__ inline uint32_t addmod(uint32_t a, uint32_t b, uint32_t n) {
    const uint32_t v = a + b;
    return v >= n ? v - n : v;
}

// The phases of a station's rotator (period N, step k: pair n of the stream takes table entry (k n) mod N)
// as a workgroup of `threads` lanes meets them: it stages chunks of P pairs by unit loads, lane u of a
// load holding pairs 2u, 2u + 1.  The steps are sums mod N from one 64-bit reduction of the call's
// first pair; k n < 2^24.
struct RotatorPhase {
    uint32_t N, k, n0;
    uint32_t tid;    // lane u's pairs 2u, 2u + 1 of a load
    uint32_t ld;     // from one load to the next
    uint32_t chunk;  // from one chunk to the next
    __device__ RotatorPhase(uint32_t N_, uint32_t k_, unsigned long long first_pair, uint32_t lane, uint32_t threads, uint32_t P)
        : N(N_), k(k_), n0((uint32_t)(first_pair % (unsigned long long)N_)),  // 64-bit reduction first
          tid((2u * k_ * lane) % N_), ld((2u * k_ * threads) % N_), chunk((k_ * (P % N_)) % N_) {}
    // phase of the pair `rel` pairs from the call's first one (rel < 0: in front of it)
    __device__ uint32_t of(long long rel) const {
        long long r = rel % (long long)N;
        if (r < 0) r += (long long)N;
        return (k * addmod(n0, (uint32_t)r, N)) % N;
    }
};

// A single-wave workgroup's LDS hand-off (mono_fused.hip chunk_sync<64>): LDS instructions of one
// wave execute in issue order; the fences keep the compiler from moving accesses across it.
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace fmrx
