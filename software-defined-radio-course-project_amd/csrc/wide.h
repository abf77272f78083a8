// wide.h — the capture stage in front of the tuner: a capture at cap_fs = rf_fs * down / up (lowest
// terms) to cf32 rows at rf_fs, one row a station.  One host design (wide_design.cpp) and one launch
// interface for its two kernels: wide.hip for up = 1 (decimation by down = 2..10), rate.hip for any
// other ratio (the polyphase down-converter).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fmrx {

constexpr int kWideMinDecim = 2, kWideMaxDecim = 10;
constexpr int kRateMinUp = 2, kRateMaxUp = 48, kRateMaxDown = 125;
constexpr int kWideMaxN = 4 * kWideMaxDecim;  // entries of the longest coarse rotation table at up = 1
constexpr int kRateMaxN = 4 * kRateMaxDown;   // of any ratio: the stride of the streams' tables in both stages
constexpr int kWideChunk = 256;               // outputs a chunk of the integer kernel
constexpr int kRateChunkLanes = 64;           // a chunk of the rational one: 64 up outputs of 64 down wide pairs
constexpr int rate_taps(int down) { return 16 * down + 1; }
// raw wide pairs of history the context keeps: ceil(16 down / up), to a whole staging unit (two pairs);
// 16 down at up = 1
constexpr int rate_hist_pairs(int up, int down) { return ((16 * down + up - 1) / up + 1) & ~1; }
// columns of history in front of a chunk in a polyphase row: ceil(16 / up)
constexpr int rate_hist_cols(int up) { return (16 + up - 1) / up; }
// floats of the taps regrouped by phase: up rows of ceil((16 down + 1) / up)
constexpr int rate_phase_stride(int up, int down) { return (rate_taps(down) + up - 1) / up; }
// columns of a polyphase row of the rational kernel's LDS buffer: the history and the chunk's 64, made
// odd (the staging stores of neighbouring rows then spread over the banks)
constexpr int rate_row_cols(int up) { return (kRateChunkLanes + rate_hist_cols(up)) | 1; }

// up / down = rf_fs / cap_fs in lowest terms.  0: a rational ratio inside the limits (2 <= up <= 48,
// up < down <= 125, down <= 10 up); 1: up = 1 (an integer ratio, *down the decimation, 1 for cap_fs =
// rf_fs); -1: anything else (rf_fs not a positive multiple of 4, cap_fs < rf_fs, a ratio outside).
int rate_ratio(int rf_fs, int cap_fs, int* up, int* down);

// Split of an offset f Hz at cap_fs = rf_fs down / up into coarse = q rf_fs / 4 (q the nearest integer
// to 4 f / rf_fs, halves away from zero) and fine = f - coarse; the coarse rotator at cap_fs has period
// N = 4 down / gcd(|q| up, 4 down) and step k = (q up / gcd) mod N.  cos_sin (may be null): 2 N floats
// c0, s0, c1, s1, ... as tuner_design makes them.  Returns false for 2 |f| >= cap_fs; the ratio and the
// fine part are the caller's to check.
bool rate_split(int rf_fs, int up, int down, int offset_hz, int* coarse_hz, int* fine_hz, int* N, int* k, float* cos_sin);

// A tap as the rational kernel reads it: the coefficient and the byte offset, in the LDS rows, of the pair
// lane 0 multiplies by it (lane t: 8 t bytes further)
struct RateTap {
    float h;
    int32_t off;
};
// The 16 down + 1 taps h regrouped by output phase: tp[phi * stride + i] is tap (phi down) mod up + up i,
// the taps of one phase contiguous in the order the sum takes them ({0, 0} behind a phase's last tap).
// Tap i of phase phi reads buffer pair HC down + t down + e - i, e = floor(phi down / up): row (e - i) mod
// down, column HC + t + floor((e - i) / down) of rows rate_row_cols(up) wide.
void rate_taps_by_phase(const float* h, int up, int down, RateTap* tp);

// One station's coarse rotator on the device: its table is tables[kRateMaxN * s ..) as (c, s) pairs.
struct WideStream {
    uint32_t N, k;
};

struct DdcLaunch {
    const uint8_t* iq;        // the ONE capture every station reads
    const uint8_t* hist;      // the rate_hist_pairs(up, down) raw pairs in front of it
    size_t stream_bytes;      // n_out * down / up pairs (whole, even), in the format's bytes
    float* y;                 // station s, output m: y[s * y_stride + 2 m], y[.. + 1]
    size_t y_stride;          // floats between rows (>= 2 n_out, a multiple of 4)
    long long n_out;          // outputs a station
    int segs;                 // workgroups a station
    int format;               // kIqU8 .. kIqF32
    int up, down;
    const WideStream* streams;  // n_streams (device)
    const float2* tables;       // n_streams x kRateMaxN (device)
    const void* taps;           // device; up = 1: the 16 down + 1 floats; otherwise: the RateTap rows by phase
    unsigned long long first_pair;  // absolute wide-pair index of the call's first pair
};

// Bytes of dynamic LDS a workgroup of the rational kernel takes: the table, the polyphase rows, the
// output hand-off.
size_t rate_lds_bytes(int up, int down);
// Workgroups a station for n_out outputs of n_streams stations on a device of `cus` compute units.
int wide_segments(long long n_out, int up, int down, int n_streams, int cus);
// up = 1: wide_ddc_kernel<down, format>; any other ratio: rate_ddc_kernel<format>.  Returns 0 on success,
// -1 for a ratio or format with no kernel, -2 on a launch error.  The capture, the history and
// stream_bytes are aligned to two pairs of the format.
int launch_wide_ddc(const DdcLaunch& L, int n_streams, hipStream_t s);
// launch_wide_ddc's two halves, arguments checked: wide.hip and rate.hip
int launch_decim_kernel(const DdcLaunch& L, int n_streams, hipStream_t s);
int launch_rate_kernel(const DdcLaunch& L, int n_streams, hipStream_t s);

}  // namespace fmrx
