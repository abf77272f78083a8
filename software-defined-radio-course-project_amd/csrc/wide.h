// wide.h — launch interface of the decimating down-converter in front of the tuner (wide.hip): the
// host design of an offset against a capture at cap_fs = decim * rf_fs, and the kernel that takes the
// capture's raw I/Q to cf32 rows at rf_fs, one row a station.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fmrx {

constexpr int kWideMinDecim = 2, kWideMaxDecim = 10;
constexpr int kWideMaxN = 4 * kWideMaxDecim;  // entries of a coarse rotation table
constexpr int wide_taps(int decim) { return 16 * decim + 1; }

// Split of an offset f Hz at cap_fs = decim * rf_fs into coarse = q rf_fs / 4 (q the nearest integer
// to 4 f / rf_fs, halves away from zero) and fine = f - coarse; the coarse rotator at cap_fs has
// period N = 4 decim / gcd(|q|, 4 decim) and step k = (q / gcd) mod N.  cos_sin (may be null): 2 N
// floats c0, s0, c1, s1, ... as tuner_design makes them.  Returns false for decim outside 2..10,
// rf_fs <= 0 or not divisible by 4, or 2 |f| >= cap_fs; the fine part is the caller's to check.
bool wide_split(int rf_fs, int decim, int offset_hz, int* coarse_hz, int* fine_hz, int* N, int* k, float* cos_sin);

// One station's coarse rotator on the device: its table is tables[kWideMaxN * s ..) as (c, s) pairs.
struct WideStream {
    uint32_t N, k;
};

struct WideLaunch {
    const uint8_t* iq;        // the ONE capture every station reads
    const uint8_t* hist;      // the 16 decim raw pairs in front of it
    size_t stream_bytes;      // n_out * decim pairs, in the format's bytes
    float* y;                 // station s, output m: y[s * y_stride + 2 m], y[.. + 1]
    size_t y_stride;          // floats between rows (>= 2 n_out, a multiple of 4)
    long long n_out;          // outputs a station
    int segs;                 // workgroups a station
    int format;               // kIqU8 .. kIqF32
    const WideStream* streams;  // n_streams (device)
    const float2* tables;       // n_streams x kWideMaxN (device)
    const float* h;             // 16 decim + 1 taps (device)
    unsigned long long first_pair;  // absolute wide-pair index of the call's first pair
};

// Workgroups a station for n_out outputs of n_streams stations on a device of `cus` compute units.
int wide_segments(long long n_out, int decim, int n_streams, int cus);
// Returns 0 on success, -1 for a decim or format with no kernel, -2 on a launch error.  The capture
// and stream_bytes are aligned to two pairs of the format.
int launch_wide_ddc(const WideLaunch& L, int n_streams, int decim, hipStream_t s);

}  // namespace fmrx
