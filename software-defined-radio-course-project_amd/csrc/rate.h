// rate.h — launch interface of the rational down-converter in front of the tuner (rate.hip): the host
// design of an offset against a capture at cap_fs = rf_fs * down / up, and the kernel that takes the
// capture's raw I/Q to cf32 rows at rf_fs, one row a station.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "wide.h"

namespace fmrx {

constexpr int kRateMinUp = 2, kRateMaxUp = 48, kRateMaxDown = 125;
constexpr int kRateMaxN = 4 * kRateMaxDown;  // entries of a coarse rotation table
constexpr int kRateChunkLanes = 64;          // a chunk: 64 up outputs of 64 down wide pairs
constexpr int rate_taps(int down) { return 16 * down + 1; }
// raw wide pairs of history the context keeps: ceil(16 down / up), to a whole staging unit (two pairs)
constexpr int rate_hist_pairs(int up, int down) { return ((16 * down + up - 1) / up + 1) & ~1; }
// columns of history in front of a chunk in a polyphase row: ceil(16 / up)
constexpr int rate_hist_cols(int up) { return (16 + up - 1) / up; }
// floats of the taps regrouped by phase: up rows of ceil((16 down + 1) / up)
constexpr int rate_phase_stride(int up, int down) { return (rate_taps(down) + up - 1) / up; }

// up / down = rf_fs / cap_fs in lowest terms.  0: a rational ratio inside the limits (2 <= up <= 48,
// up < down <= 125, down <= 10 up); 1: up = 1 (an integer ratio, *down the decimation, 1 for cap_fs =
// rf_fs); -1: anything else (rf_fs not a positive multiple of 4, cap_fs < rf_fs, a ratio outside).
int rate_ratio(int rf_fs, int cap_fs, int* up, int* down);

// Split of an offset f Hz at cap_fs = rf_fs down / up into coarse = q rf_fs / 4 (wide_split's q) and
// fine = f - coarse; the coarse rotator at cap_fs has period N = 4 down / gcd(|q| up, 4 down) and step
// k = (q up / gcd) mod N.  cos_sin (may be null): 2 N floats as tuner_design makes them.  Returns false
// for 2 |f| >= cap_fs; the ratio and the fine part are the caller's to check.
bool rate_split(int rf_fs, int up, int down, int offset_hz, int* coarse_hz, int* fine_hz, int* N, int* k, float* cos_sin);

// columns of a polyphase row of the kernel's LDS buffer: the history and the chunk's 64, made odd (the
// staging stores of neighbouring rows then spread over the banks)
constexpr int rate_row_cols(int up) { return (kRateChunkLanes + rate_hist_cols(up)) | 1; }

// A tap as the kernel reads it: the coefficient and the byte offset, in the LDS rows, of the pair lane 0
// multiplies by it (lane t: 8 t bytes further)
struct RateTap {
    float h;
    int32_t off;
};
// The 16 down + 1 taps h regrouped by output phase: tp[phi * stride + i] is tap (phi down) mod up + up i,
// the taps of one phase contiguous in the order the sum takes them ({0, 0} behind a phase's last tap).
// Tap i of phase phi reads buffer pair HC down + t down + e - i, e = floor(phi down / up): row (e - i) mod
// down, column HC + t + floor((e - i) / down) of rows rate_row_cols(up) wide.
void rate_taps_by_phase(const float* h, int up, int down, RateTap* tp);

struct RateLaunch {
    const uint8_t* iq;        // the ONE capture every station reads
    const uint8_t* hist;      // the rate_hist_pairs raw pairs in front of it
    size_t stream_bytes;      // n_out * down / up pairs (whole, even), in the format's bytes
    float* y;                 // station s, output m: y[s * y_stride + 2 m], y[.. + 1]
    size_t y_stride;          // floats between rows (>= 2 n_out)
    long long n_out;          // outputs a station
    int segs;                 // workgroups a station
    int format;               // kIqU8 .. kIqF32
    int up, down;
    const WideStream* streams;  // n_streams (device)
    const float2* tables;       // n_streams x kRateMaxN (device)
    const RateTap* hp;          // the taps by phase (device)
    unsigned long long first_pair;  // absolute wide-pair index of the call's first pair
};

// Bytes of dynamic LDS a workgroup takes: the table, the polyphase rows, the output hand-off.
size_t rate_lds_bytes(int up, int down);
// Workgroups a station for n_out outputs of n_streams stations on a device of `cus` compute units.
int rate_segments(long long n_out, int up, int down, int n_streams, int cus);
// Returns 0 on success, -1 for a ratio or format with no kernel, -2 on a launch error.  The capture,
// the history and stream_bytes are aligned to two pairs of the format.
int launch_rate_ddc(const RateLaunch& L, int n_streams, hipStream_t s);

}  // namespace fmrx
