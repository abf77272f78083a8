// scan.h — launch interface of the band scan's spectrum kernels (scan.hip): the Welch power
// spectrum of a raw I/Q capture.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fmrx {

constexpr int kScanMinBins = 256, kScanMaxBins = 8192;

inline bool scan_bins_ok(int n) { return n >= kScanMinBins && n <= kScanMaxBins && (n & (n - 1)) == 0; }

// Host tables of an N-point scan, computed in double and rounded once: tw = N (re, im) pairs,
// tw[k] = exp(-2 pi j k / N); win = N floats, the periodic Hann window 0.5 - 0.5 cos(2 pi i / N).
void scan_tables(int N, float* tw, float* win);

// Partial rows (workgroups) a launch over nseg segments of N bins uses on a device of `cus` compute
// units (format: the instantiation's occupancy): at most nseg, so every row is written.  0 on a HIP error.
int scan_workgroups(int N, size_t nseg, int cus, int format);

// power[j] (N floats, FFT-shifted) of segments [0, nseg) of iq (format: tuner.h kIqU8 .. kIqF32; aligned
// to one pair of it), as fmrx.h defines it.  part: scratch of G * N floats, G = scan_workgroups(...) of
// the same format.  Returns 0, -1 (bad N or format) or -2 (launch error).
int launch_scan(const uint8_t* iq, int format, size_t nseg, int N, const float* d_tw, const float* d_win, float* d_part,
                int G, float* d_power, hipStream_t s);

}  // namespace fmrx
