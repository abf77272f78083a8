// wide_design.cpp — host side of the capture stage (wide.h): the ratio of a capture rate, the split of
// an offset and its coarse rotator, the rational kernel's taps by phase, the workgroup counts and the
// dispatch to the stage's two kernels.  Nothing here runs on the device.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "wide.h"

namespace fmrx {

int rate_ratio(int rf_fs, int cap_fs, int* up, int* down) {
    if (rf_fs <= 0 || rf_fs % 4 != 0 || cap_fs < rf_fs) return -1;
    const int g = std::gcd(rf_fs, cap_fs);
    const int l = rf_fs / g, m = cap_fs / g;
    if (l == 1) {
        if (up) *up = 1;
        if (down) *down = m;
        return 1;
    }
    if (l < kRateMinUp || l > kRateMaxUp || m <= l || m > kRateMaxDown || m > 10 * l) return -1;
    if (up) *up = l;
    if (down) *down = m;
    return 0;
}

bool rate_split(int rf_fs, int up, int down, int offset_hz, int* coarse_hz, int* fine_hz, int* N, int* k, float* cos_sin) {
    const long long fs = rf_fs, f = offset_hz, a = f < 0 ? -f : f;
    if (2 * a * up >= fs * down) return false;  // 2 |f| >= cap_fs
    const long long qa = (8 * a + fs) / (2 * fs), q = f < 0 ? -qa : qa;
    const long long fc = q * (fs / 4);
    const long long g = std::gcd(qa * up, (long long)(4 * down));  // gcd(0, 4 M) = 4 M: N = 1, k = 0
    const long long n = 4 * down / g;
    const long long kk = ((q * up / g) % n + n) % n;
    if (coarse_hz) *coarse_hz = (int)fc;
    if (fine_hz) *fine_hz = (int)(f - fc);
    if (N) *N = (int)n;
    if (k) *k = (int)kk;
    if (cos_sin) {
        for (long long p = 0; p < n; p++) {  // the angle as (2 pi p) / N, one rounding each
            const double ang = (2.0 * 3.14159265358979323846 * (double)p) / (double)n;
            cos_sin[2 * p] = (float)std::cos(ang);
            cos_sin[2 * p + 1] = (float)std::sin(ang);
        }
    }
    return true;
}

void rate_taps_by_phase(const float* h, int up, int down, RateTap* tp) {
    const int ts = rate_phase_stride(up, down), taps = rate_taps(down);
    const int hc = rate_hist_cols(up), w = rate_row_cols(up);
    for (int phi = 0; phi < up; phi++) {
        const int e = phi * down / up, k0 = phi * down - e * up;
        for (int i = 0; i < ts; i++) {
            const int kk = k0 + up * i;
            const int u = hc * down + e - i;  // >= 0 for every tap there is
            tp[phi * ts + i] = kk < taps ? RateTap{h[kk], (int32_t)sizeof(float2) * ((u % down) * w + u / down)} : RateTap{0.0f, 0};
        }
    }
}

size_t rate_lds_bytes(int up, int down) {
    return sizeof(float2) * ((size_t)kRateMaxN + (size_t)down * rate_row_cols(up) + (size_t)kRateChunkLanes * (up | 1));
}

int wide_segments(long long n_out, int up, int down, int n_streams, int cus) {
    // outputs a chunk, a workgroup's LDS and the waves the registers leave a SIMD: the integer kernel
    // (one wave a workgroup, at most two a SIMD) and the rational one (four waves, at most six a SIMD)
    const bool integer = up == 1;
    const long long cm = integer ? kWideChunk : (long long)kRateChunkLanes * up;
    const long long lds = integer ? 8 * (down * (16 + kWideChunk + 1) + kWideMaxN) : (long long)rate_lds_bytes(up, down);
    const long long chunks = (n_out + cm - 1) / cm;
    // resident workgroups a CU: 160 KiB of LDS
    const long long target_wg =
        (long long)std::max(1, cus) * std::min<long long>(integer ? 8 : 6, std::max<long long>(1, 160 * 1024 / lds));
    // tuner_segments' rule: one wave of workgroups, segments of at least four chunks, and a call
    // too short to fill the grid even so takes one chunk a segment
    if ((long long)n_streams * chunks <= target_wg) return (int)std::max<long long>(1, chunks);
    long long segs = std::max<long long>(1, target_wg / std::max(1, n_streams));
    segs = std::min(segs, std::max<long long>(1, chunks / 4));
    return (int)segs;
}

int launch_wide_ddc(const DdcLaunch& L, int n_streams, hipStream_t s) {
    if (L.segs < 1 || n_streams < 1 || L.n_out < 1) return -1;
    if (L.up == 1) return launch_decim_kernel(L, n_streams, s);
    if (L.up < kRateMinUp || L.up > kRateMaxUp || L.down <= L.up || L.down > kRateMaxDown || L.down > 10 * L.up) return -1;
    return launch_rate_kernel(L, n_streams, s);
}

}  // namespace fmrx
