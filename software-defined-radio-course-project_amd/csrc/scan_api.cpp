// scan_api.cpp — the spectrum calls: the PSD estimate (spectrum.hip), the band scan's Welch spectrum
// of a raw capture (scan.hip) and its station detector, which runs on the host.
#include <cmath>

#include "ctx.h"
#include "scan.h"

using namespace fmrx;

extern "C" {

// ---- PSD estimate ------------------------------------------------------
namespace {
// estimatePSD's window (fourier.cpp:57-61): pow(sin(i*PI/N), 2) in double, stored as float.
int psd_run(fmrx_ctx* c, const float* d_x, size_t n, int freq_bins, float fs, float* d_psd) {
    const int N = freq_bins;
    if (N < 2 || N > kPsdMaxBins || (N & (N - 1)) != 0)
        return fail(FMRX_EINVAL, "freq_bins must be a power of two in [2, %d]", kPsdMaxBins);
    const size_t nseg = n / (size_t)N;
    if (nseg < 1) return fail(FMRX_EINVAL, "need at least freq_bins samples");
    int rc = c->io.scratch.ensure((size_t)N + nseg * (N / 2));
    if (rc) return rc;
    std::vector<float> hann(N);
    for (int i = 0; i < N; i++) {
        const double s = std::sin(i * 3.14159265358979323846 / N);  // PI, dy4.h:14
        hann[i] = (float)(s * s);
    }
    HIPCHK(hipMemcpyAsync(c->io.scratch.p, hann.data(), sizeof(float) * N, hipMemcpyHostToDevice, c->stream));
    // psd_seg = (4 / (Fs * freq_bins)) * |X|^2 (fourier.cpp:103)
    const double scale = 4.0 / ((double)fs * (double)N);
    if (launch_psd(d_x, (int)nseg, N, c->io.scratch.p, scale, c->io.scratch.p + N, d_psd, c->stream))
        return fail(FMRX_EHIP, "PSD launch failed");
    HIPCHK(hipStreamSynchronize(c->stream));  // the window lives in host memory until here
    return 0;
}
}  // namespace

int fmrx_psd_device(fmrx_ctx* c, const float* d_samples, size_t n, int freq_bins, float fs, float* d_psd) {
    CtxLock lock_(c);
    if (!c || !d_samples || !d_psd) return fail(FMRX_EINVAL, "null argument");
    int rc = set_device(c);
    return rc ? rc : psd_run(c, d_samples, n, freq_bins, fs, d_psd);
}

int fmrx_estimate_psd(fmrx_ctx* c, const float* samples, size_t n, int freq_bins, float fs, float* freq,
                      float* psd) {
    CtxLock lock_(c);
    if (!c || !samples || !freq || !psd) return fail(FMRX_EINVAL, "null argument");
    int rc = set_device(c);
    if (rc) return rc;
    if (freq_bins < 2) return fail(FMRX_EINVAL, "freq_bins must be >= 2");
    const size_t used = n / (size_t)freq_bins * (size_t)freq_bins;
    if ((rc = c->io.f32.ensure(used + (size_t)freq_bins / 2))) return rc;
    HIPCHK(hipMemcpyAsync(c->io.f32.p, samples, sizeof(float) * used, hipMemcpyHostToDevice, c->stream));
    if ((rc = psd_run(c, c->io.f32.p, used, freq_bins, fs, c->io.f32.p + used))) return rc;
    HIPCHK(hipMemcpy(psd, c->io.f32.p + used, sizeof(float) * (freq_bins / 2), hipMemcpyDeviceToHost));
    const float df = fs / (float)freq_bins;  // fourier.cpp:42-50
    for (int i = 0; i < freq_bins / 2; i++) freq[i] = (float)i * df;
    return FMRX_OK;
}

// ---- band scan: Welch spectrum of the raw capture (scan.hip) + the host station detector -----
int fmrx_scan_config_default(fmrx_scan_config* cfg) {
    if (!cfg) return fail(FMRX_EINVAL, "null config");
    *cfg = fmrx_scan_config{4096, 100000, 0, 150000, 200000, 1, 25, 10.0f};
    return FMRX_OK;
}

namespace {
int scan_check_size(int fft_bins, size_t n_pairs) {
    if (!scan_bins_ok(fft_bins))
        return fail(FMRX_EINVAL, "fft_bins %d: need a power of two in [%d, %d]", fft_bins, kScanMinBins, kScanMaxBins);
    if (n_pairs < (size_t)fft_bins) return fail(FMRX_EINVAL, "%zu I/Q pairs: fewer than fft_bins (%d)", n_pairs, fft_bins);
    if (n_pairs / (size_t)fft_bins > 0xffffffffu) return fail(FMRX_EINVAL, "capture too long");
    return 0;
}

// arguments checked, device set; enqueues on the context stream
int scan_run(fmrx_ctx* c, const uint8_t* d_iq, size_t n_pairs, int N, float* d_power) {
    int rc;
    const size_t nseg = n_pairs / (size_t)N;
    if (c->scan.bins != N) {  // tables of this size: stream-ordered behind a scan still in flight
        c->scan.bins = 0;
        HIPCHK(hipStreamSynchronize(c->stream));  // the host copy is replaced below
        c->scan.tab_host.resize(3 * (size_t)N);
        scan_tables(N, c->scan.tab_host.data(), c->scan.tab_host.data() + 2 * (size_t)N);
        if ((rc = c->scan.tab.ensure(3 * (size_t)kScanMaxBins))) return rc;
        HIPCHK(hipMemcpyAsync(c->scan.tab.p, c->scan.tab_host.data(), sizeof(float) * c->scan.tab_host.size(),
                              hipMemcpyHostToDevice, c->stream));
        c->scan.bins = N;
    }
    if (reinterpret_cast<uintptr_t>(d_iq) % c->front.pair_bytes != 0)
        return fail(FMRX_EINVAL, "scan: the capture must be aligned to one %zu-byte I/Q pair", c->front.pair_bytes);
    const int G = scan_workgroups(N, nseg, c->n_simd / 4, c->front.format);
    if (G < 1) return fail(FMRX_EHIP, "scan: no resident workgroup for %d bins", N);
    if ((rc = c->scan.part.ensure((size_t)G * N))) return rc;
    rc = launch_scan(d_iq, c->front.format, nseg, N, c->scan.tab.p, c->scan.tab.p + 2 * (size_t)N, c->scan.part.p, G, d_power,
                     c->stream);
    if (rc) return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "scan launch failed");
    return 0;
}
}  // namespace

int fmrx_scan_spectrum_device(fmrx_ctx* c, const uint8_t* d_iq, size_t n_pairs, int fft_bins, float* d_power) {
    CtxLock lock_(c);
    if (!c || !d_iq || !d_power) return fail(FMRX_EINVAL, "null argument");
    int rc = scan_check_size(fft_bins, n_pairs);
    if (rc || (rc = set_device(c))) return rc;
    return scan_run(c, d_iq, n_pairs, fft_bins, d_power);
}

int fmrx_scan_spectrum(fmrx_ctx* c, const uint8_t* iq, size_t n_pairs, int fft_bins, float* power, size_t* n_segments) {
    CtxLock lock_(c);
    if (!c || !iq || !power) return fail(FMRX_EINVAL, "null argument");
    int rc = scan_check_size(fft_bins, n_pairs);
    if (rc || (rc = set_device(c))) return rc;
    const size_t nseg = n_pairs / (size_t)fft_bins, bytes = c->front.pair_bytes * nseg * (size_t)fft_bins;
    if ((rc = c->scan.in.ensure(bytes)) || (rc = c->scan.power.ensure(kScanMaxBins))) return rc;
    HIPCHK(hipMemcpyAsync(c->scan.in.p, iq, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = scan_run(c, c->scan.in.p, nseg * (size_t)fft_bins, fft_bins, c->scan.power.p))) return rc;
    std::vector<float> got((size_t)fft_bins);  // the caller's buffer is written only on success
    HIPCHK(hipMemcpyAsync(got.data(), c->scan.power.p, sizeof(float) * fft_bins, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::copy(got.begin(), got.end(), power);
    if (n_segments) *n_segments = nseg;
    return FMRX_OK;
}

namespace {
// The scan configuration a call runs with: the defaults, or the caller's
fmrx_scan_config scan_config_of(const fmrx_scan_config* cfg_in) {
    fmrx_scan_config cfg;
    (void)fmrx_scan_config_default(&cfg);
    return cfg_in ? *cfg_in : cfg;
}

// The detector of fmrx_scan_detect, fmrx_scan_detect_wide and fmrx_scan_detect_rate on the spectrum of a
// capture at rf_fs for a mode at mode_fs.  A candidate is one the receiver can tune to: at the mode's own
// rate fmrx_tuner_design accepts it, at any other fmrx_rate_design does (an integer ratio: with
// fmrx_wide_design's answer).  Host arrays in and out: nothing here touches the GPU.
int scan_detect_run(const float* power, int fft_bins, int rf_fs, int mode_fs, const fmrx_scan_config& cfg, fmrx_station* out,
                    int max_out, int* n_found, float* floor_db) {
    if (!power || !n_found || max_out < 0 || (max_out > 0 && !out)) return fail(FMRX_EINVAL, "bad argument");
    const int N = fft_bins;
    if (!scan_bins_ok(N))
        return fail(FMRX_EINVAL, "fft_bins %d: need a power of two in [%d, %d]", N, kScanMinBins, kScanMaxBins);
    if (rf_fs <= 0 || cfg.raster_hz <= 0 || cfg.channel_hz <= 0 || cfg.min_separation_hz <= 0)
        return fail(FMRX_EINVAL, "rf_fs, raster_hz, channel_hz and min_separation_hz must be positive");
    if (cfg.channel_hz >= rf_fs) return fail(FMRX_EINVAL, "channel_hz %d is not below rf_fs %d", cfg.channel_hz, rf_fs);
    if (cfg.floor_percentile < 1 || cfg.floor_percentile > 99)
        return fail(FMRX_EINVAL, "floor_percentile %d outside 1..99", cfg.floor_percentile);
    if (cfg.dc_notch_bins < 0 || cfg.dc_notch_bins > N / 2)
        return fail(FMRX_EINVAL, "dc_notch_bins %d outside [0, fft_bins / 2]", cfg.dc_notch_bins);
    // candidates f_m = origin + m raster with 2 |f_m| + channel_hz <= rf_fs, ascending
    const long long fs = rf_fs, ch = cfg.channel_hz, ras = cfg.raster_hz, org = cfg.raster_origin_hz;
    const long long reach = (fs - ch) / 2;  // |f_m| <= (rf_fs - channel_hz) / 2, f_m an integer
    auto floor_div = [](long long a, long long b) { return a / b - ((a % b != 0 && (a % b < 0) != (b < 0)) ? 1 : 0); };
    const long long m_lo = -floor_div(reach + org, ras), m_hi = floor_div(reach - org, ras);
    struct Cand {
        long long f;
        double c;
        int nb;
        double snr;
    };
    std::vector<Cand> cands;
    for (long long m = m_lo; m <= m_hi; m++) {
        const long long f = org + m * ras;
        int tn = 0, tk = 0;
        // every reported offset can be tuned to
        const int rc = mode_fs == rf_fs ? fmrx_tuner_design(rf_fs, (int)f, &tn, &tk, nullptr)
                                        : fmrx_rate_design(mode_fs, rf_fs, (int)f, nullptr, nullptr, nullptr, nullptr, &tn, &tk, nullptr, nullptr, nullptr);
        if (rc) return rc;
        cands.push_back(Cand{f, 0.0, 0, 0.0});
    }
    // noise floor: a percentile of the kept bins
    std::vector<double> p((size_t)N), kept;
    kept.reserve((size_t)N);
    auto is_kept = [&](int j) { return std::abs(j - N / 2) >= cfg.dc_notch_bins; };
    for (int j = 0; j < N; j++) {
        p[j] = std::max((double)power[j], 1e-20);
        if (is_kept(j)) kept.push_back(p[j]);
    }
    if (kept.empty()) return fail(FMRX_EINVAL, "dc_notch_bins %d leaves no bin", cfg.dc_notch_bins);
    std::sort(kept.begin(), kept.end());
    const double floor_p = kept[((size_t)cfg.floor_percentile * (kept.size() - 1)) / 100];
    for (Cand& cd : cands) {
        for (int j = 0; j < N; j++) {
            if (!is_kept(j)) continue;
            long long d = (long long)(j - N / 2) * fs - cd.f * N;
            if (d < 0) d = -d;
            if (2 * d <= ch * N) {
                cd.c += p[j];
                cd.nb++;
            }
        }
        cd.snr = cd.nb ? 10.0 * std::log10(cd.c / (floor_p * cd.nb)) : 0.0;
    }
    // strongest first (ties: lower offset); a candidate with no kept bin is never reported
    std::vector<const Cand*> order;
    for (const Cand& cd : cands)
        if (cd.nb) order.push_back(&cd);
    std::stable_sort(order.begin(), order.end(), [](const Cand* a, const Cand* b) { return a->c > b->c; });
    std::vector<const Cand*> acc;
    for (const Cand* cd : order) {
        if (!(cd->snr >= (double)cfg.min_snr_db)) continue;
        bool clear = true;
        for (const Cand* a : acc) {
            const long long d = cd->f > a->f ? cd->f - a->f : a->f - cd->f;
            if (d < cfg.min_separation_hz) clear = false;
        }
        if (clear) acc.push_back(cd);
    }
    *n_found = (int)acc.size();
    if (floor_db) *floor_db = (float)(10.0 * std::log10(floor_p));
    if (acc.size() > (size_t)max_out) acc.resize((size_t)max_out);
    std::sort(acc.begin(), acc.end(), [](const Cand* a, const Cand* b) { return a->f < b->f; });
    for (size_t i = 0; i < acc.size(); i++)
        out[i] = fmrx_station{(int32_t)acc[i]->f, (float)(10.0 * std::log10(acc[i]->c)), (float)acc[i]->snr};
    return FMRX_OK;
}

// fmrx_scan and fmrx_scan_wide: spectrum + detect at the rate of the capture
int scan_both(fmrx_ctx* c, const uint8_t* iq, size_t n_pairs, int fs, const fmrx_scan_config* cfg_in, fmrx_station* out,
              int max_out, int* n_found) {
    const fmrx_scan_config cfg = scan_config_of(cfg_in);
    const int mode_fs = c->geo.rf_fs;
    int rc = scan_check_size(cfg.fft_bins, n_pairs);
    if (rc) return rc;
    {  // refuse a bad detector configuration before any GPU work
        std::vector<float> flat((size_t)cfg.fft_bins, 1.0f);
        std::vector<fmrx_station> tmp((size_t)std::max(max_out, 0));
        int n = 0;
        if ((rc = scan_detect_run(flat.data(), cfg.fft_bins, fs, mode_fs, cfg, tmp.data(), max_out, &n, nullptr))) return rc;
    }
    std::vector<float> power((size_t)cfg.fft_bins);
    if ((rc = fmrx_scan_spectrum(c, iq, n_pairs, cfg.fft_bins, power.data(), nullptr))) return rc;
    return scan_detect_run(power.data(), cfg.fft_bins, fs, mode_fs, cfg, out, max_out, n_found, nullptr);
}
}  // namespace

int fmrx_scan_detect(const float* power, int fft_bins, int rf_fs, const fmrx_scan_config* cfg_in, fmrx_station* out,
                     int max_out, int* n_found, float* floor_db) {
    return scan_detect_run(power, fft_bins, rf_fs, rf_fs, scan_config_of(cfg_in), out, max_out, n_found, floor_db);
}

int fmrx_scan_detect_wide(const float* power, int fft_bins, int rf_fs, int decim, const fmrx_scan_config* cfg_in,
                          fmrx_station* out, int max_out, int* n_found, float* floor_db) {
    int rc = check_capture_decim(decim, false);
    if (rc || (rc = check_wide_rf_fs(rf_fs))) return rc;
    return scan_detect_run(power, fft_bins, rf_fs * decim, rf_fs, scan_config_of(cfg_in), out, max_out, n_found, floor_db);
}

int fmrx_scan_detect_rate(const float* power, int fft_bins, int rf_fs, int cap_fs, const fmrx_scan_config* cfg_in,
                          fmrx_station* out, int max_out, int* n_found, float* floor_db) {
    int rc = fmrx_rate_design(rf_fs, cap_fs, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;  // the rate itself
    return scan_detect_run(power, fft_bins, cap_fs, rf_fs, scan_config_of(cfg_in), out, max_out, n_found, floor_db);
}

int fmrx_scan_wide(fmrx_ctx* c, const uint8_t* iq, size_t n_pairs, const fmrx_scan_config* cfg_in, fmrx_station* out,
                   int max_out, int* n_found) {
    CtxLock lock_(c);
    if (!c || !iq || !n_found) return fail(FMRX_EINVAL, "null argument");
    if (!c->wide.ratio.on()) return fail(FMRX_ESTATE, "fmrx_scan_wide: the capture decimation is 1 (fmrx_set_capture_decim first)");
    return scan_both(c, iq, n_pairs, c->wide.ratio.cap_fs(c->geo.rf_fs), cfg_in, out, max_out, n_found);
}

int fmrx_scan(fmrx_ctx* c, const uint8_t* iq, size_t n_pairs, const fmrx_scan_config* cfg_in, fmrx_station* out,
              int max_out, int* n_found) {
    CtxLock lock_(c);
    if (!c || !iq || !n_found) return fail(FMRX_EINVAL, "null argument");
    // kept as it was: on a context at a rational rate this call has always scanned at the capture's rate,
    // as fmrx_scan_wide does, and at rf_fs on every other (fmrx.h promises rf_fs throughout)
    const int fs = c->wide.ratio.rational() ? c->wide.ratio.cap_fs(c->geo.rf_fs) : c->geo.rf_fs;
    return scan_both(c, iq, n_pairs, fs, cfg_in, out, max_out, n_found);
}

}  // extern "C"
