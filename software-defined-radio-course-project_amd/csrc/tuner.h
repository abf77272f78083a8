// tuner.h — launch interface of the frequency-translating front end (tuner.hip): the rotator
// design (host) and the kernel that takes raw I/Q (u8, s8, s16 or f32 pairs) to demod rows for a
// per-stream offset.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mono_launch.h"

namespace fmrx {

constexpr int kTunerMaxN = 4096;  // rotator period in pairs: a table of at most 32 KiB a stream

// Raw I/Q formats (include/fmrx.h FMRX_IQ_*): bytes an I/Q pair, -1 for an unknown format
constexpr int kIqU8 = 0, kIqS8 = 1, kIqS16 = 2, kIqF32 = 3;
constexpr int iq_pair_bytes(int format) {
    return format == kIqU8 || format == kIqS8 ? 2 : format == kIqS16 ? 4 : format == kIqF32 ? 8 : -1;
}

// Rotator of an offset f Hz at rf_fs: period N = rf_fs / gcd(|f|, rf_fs) pairs, step
// k = (f / gcd) mod N, pair n takes table entry (k n) mod N.  Returns false when |f| >= rf_fs / 2
// (why = 1) or N > kTunerMaxN (why = 2).  cos_sin (may be null): the 2 N floats c[0], s[0], c[1],
// s[1], ... with c[p] = (float)cos(2 pi p / N), s[p] = (float)sin(2 pi p / N), cos and sin in double.
bool tuner_design(int rf_fs, int offset_hz, int* N, int* k, float* cos_sin, int* why = nullptr);

// One stream's rotator on the device: its table is tables[tab .. tab + N) as (c, s) pairs.
struct TunerStream {
    uint32_t N, k, tab, pad;
};

struct TunerLaunch {
    const uint8_t* iq;          // stream s at iq + s * iq_stride; iq_stride = 0: one capture for all
    size_t iq_stride;
    const uint8_t* halo;        // n_streams x halo_bytes: the bytes preceding this call, per stream
    uint8_t* halo_next;         // n_streams x halo_bytes: the halo after this call (written here)
    size_t halo_bytes;          // halo_pairs * pair_bytes
    size_t stream_bytes;        // n_blocks * iq_pairs * pair_bytes
    float* demod;               // IF sample g of stream s at demod[s * demod_stride + demod_hist + g]
    size_t demod_stride;
    int demod_hist;
    int pre_tail;               // 1: the 50 demod samples in front of the call too, at demod_hist - 50
                                //   (>= 0) .. demod_hist - 1 (the mono audio history after fmrx_seek)
    long long n_if;             // IF samples per stream this call
    int segs;                   // workgroups (segments) per stream
    int format;                 // kIqU8 .. kIqF32: iq, halo, iq_stride and both counts in its bytes
    const TunerStream* streams; // n_streams (device)
    const float2* tables;       // the streams' tables (device)
    unsigned long long first_pair;  // absolute pair index of the call's first I/Q pair
};

bool tuner_supported(int rf_taps, int rf_decim);
// Segments a stream for n_if IF samples of n_streams streams on a device of `cus` compute units,
// max_n the longest rotator period among the streams (its table sits in LDS beside the samples).
int tuner_segments(long long n_if, int rf_taps, int rf_decim, int n_streams, int cus, int max_n);
// Returns 0 on success, -1 if no compiled variant matches, -2 on a launch error.  L.halo and
// L.halo_next must be different buffers; the input rows and stream_bytes are aligned to two pairs
// of the format (4, 4, 8, 16 bytes).
int launch_tuner(const TunerLaunch& L, int n_streams, int rf_taps, int rf_decim, int max_n, const MonoTaps& taps,
                 hipStream_t s);

}  // namespace fmrx
