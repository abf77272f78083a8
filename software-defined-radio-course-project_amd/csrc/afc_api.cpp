// afc_api.cpp — AFC's entry points: the carrier sums over demod rows (afc.hip), the
// host-side report and decision, and the switch that runs the sums inside the calls whose front end writes
// demod rows, decides per stream and retunes the context between calls.
#include <cmath>

#include "ctx.h"

using namespace fmrx;

namespace {

// the kernel over the rows at d_demod (whole frames) into d_sums, enqueued
int run_carrier(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_blocks, float* d_sums) {
    int P = 0;
    if (!meter_design(c->geo.bp_fs, &P, nullptr)) return fail(FMRX_EINVAL, "no frame at bp_fs %d", c->geo.bp_fs);
    const size_t frames = meter_frames(c, n_blocks);
    if (frames > 0x7FFFFFFFull) return fail(FMRX_EINVAL, "%zu blocks: too many frames for one carrier call", n_blocks);
    CarrierLaunch L{};
    L.demod = d_demod;
    L.demod_stride = demod_stride;
    L.P = P;
    L.frames = (int)frames;
    L.sums = d_sums;
    const int rc = launch_carrier(L, c->cfg.n_streams, c->stream);
    return rc ? launch_failed(rc, "carrier", ": rows 16-byte aligned?") : 0;
}

bool config_ok(const fmrx_afc_config& k) {
    return k.step_hz > 0 && k.frames > 0 && k.max_pull_hz > 0 && k.deadband_hz >= 0 && std::isfinite(k.max_mean_square) &&
           k.max_mean_square > 0.0f;
}

// the offsets AFC moves: fmrx_tune_wide's once it was accepted, else fmrx_tune's
inline std::vector<int32_t>& offsets_of(fmrx_ctx* c) { return c->wide.tuned ? c->wide.offsets : c->tune.offsets; }
inline const std::vector<int32_t>& offsets_of(const fmrx_ctx* c) { return c->wide.tuned ? c->wide.offsets : c->tune.offsets; }

// all streams to `to` at the context's current position, through fmrx_tune's (fmrx_tune_wide's) own code
int retune(fmrx_ctx* c, const std::vector<int32_t>& to) {
    if (!c->wide.tuned) return tune_narrow(c, to.data(), c->tune.pos);
    const CaptureRatio& r = c->wide.ratio;
    return tune_wide(c, to.data(), c->tune.pos / (uint64_t)r.up * (uint64_t)r.down);  // fmrx_wide_info's position
}

// would fmrx_tune (fmrx_tune_wide) take this offset
bool design_accepts(const fmrx_ctx* c, int32_t hz) {
    if (!c->wide.tuned) return fmrx_tuner_design(c->geo.rf_fs, hz, nullptr, nullptr, nullptr) == FMRX_OK;
    return fmrx_rate_design(c->geo.rf_fs, c->wide.ratio.cap_fs(c->geo.rf_fs), hz, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, nullptr) == FMRX_OK;
}

// every stream whose window is full decides; the streams that moved are retuned together
int track(fmrx_ctx* c) {
    auto& a = c->afc;
    const size_t ns = c->cfg.n_streams;
    std::vector<int32_t> to = offsets_of(c);
    std::vector<size_t> movers;
    if (!a.moved) {  // nothing pulled yet: the origins are where the streams are
        a.origin = to;
        a.wide = c->wide.tuned;
    }
    for (size_t s = 0; s < ns; s++) {
        if (a.window[s].frames < (uint64_t)a.cfg.frames) continue;
        fmrx_afc_decision d{};
        const int rc = fmrx_afc_decide(&a.window[s], c->geo.bp_fs, &a.cfg, &d);
        if (rc) return rc;
        a.window[s] = fmrx_carrier_report{};
        a.last[s] = d;
        a.decisions[s]++;
        const int64_t lo = (int64_t)a.origin[s] - a.cfg.max_pull_hz, hi = (int64_t)a.origin[s] + a.cfg.max_pull_hz;
        const int32_t want = (int32_t)std::min(hi, std::max(lo, (int64_t)to[s] + d.correction_hz));
        if (want == to[s]) continue;
        if (!design_accepts(c, want)) {
            a.refused[s]++;
            continue;
        }
        to[s] = want;
        movers.push_back(s);
    }
    if (movers.empty()) return 0;
    const int rc = retune(c, to);
    if (rc) return rc;
    for (size_t s : movers) a.retunes[s]++;
    a.moved = true;
    return 0;
}

}  // namespace

namespace fmrx {

void reset_afc_reports(fmrx_ctx* c) {
    auto& a = c->afc;
    const size_t ns = c->cfg.n_streams;
    a.total.assign(ns, fmrx_carrier_report{});  // sized here: creation resets
    a.window.assign(ns, fmrx_carrier_report{});
    a.retunes.assign(ns, 0);
    a.refused.assign(ns, 0);
    a.decisions.assign(ns, 0);
    a.last.assign(ns, fmrx_afc_decision{});
    a.origin.resize(ns, 0);
    a.pending = 0;
}

// fmrx_reset: the offsets back to the origins (a retune at the reset's position), the reports cleared.  Origins
// of the other kind than the context's tuning now is (the capture stage changed since) are dropped instead.
int reset_afc(fmrx_ctx* c) {
    auto& a = c->afc;
    reset_afc_reports(c);
    if (!a.moved) return 0;
    a.moved = false;
    if (a.wide != c->wide.tuned || !c->tune.on) {
        a.origin = offsets_of(c);
        a.wide = c->wide.tuned;
        return 0;
    }
    return retune(c, a.origin);
}

void afc_caller_tuned(fmrx_ctx* c) {
    auto& a = c->afc;
    a.origin = offsets_of(c);
    a.wide = c->wide.tuned;
    a.moved = false;
    a.window.assign((size_t)c->cfg.n_streams, fmrx_carrier_report{});
}

int afc_enqueue(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_blocks) {
    const size_t ns = c->cfg.n_streams, frames = meter_frames(c, n_blocks);
    c->afc.pending = 0;
    int rc;
    if ((rc = c->afc.sums.ensure(ns * frames * 2))) return rc;
    if ((rc = run_carrier(c, d_demod, demod_stride, n_blocks, c->afc.sums.p))) return rc;
    c->afc.pending = frames;
    return 0;
}

int afc_finish(fmrx_ctx* c) {
    auto& a = c->afc;
    const size_t ns = c->cfg.n_streams, frames = a.pending;
    if (frames == 0) return 0;
    a.pending = 0;
    a.host.resize(ns * frames * 2);
    HIPCHK(hipMemcpyAsync(a.host.data(), a.sums.p, sizeof(float) * a.host.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t s = 0; s < ns; s++) {
        const float* row = a.host.data() + s * frames * 2;
        int rc = fmrx_carrier_accumulate(&a.total[s], row, frames);
        if (rc || (rc = fmrx_carrier_accumulate(&a.window[s], row, frames))) return rc;
    }
    return a.cfg.track ? track(c) : 0;
}

}  // namespace fmrx

extern "C" {

int fmrx_carrier_device(fmrx_ctx* c, const float* d_demod, size_t n_blocks, float* d_sums) {
    CtxLock lock_(c);
    if (!c || !d_demod || !d_sums) return fail(FMRX_EINVAL, "null argument");
    int rc = check_frame_blocks(c, n_blocks, "a carrier call");
    if (rc || n_blocks == 0) return rc;
    if ((rc = set_device(c))) return rc;
    return run_carrier(c, d_demod, n_blocks * c->geo.if_samples, n_blocks, d_sums);
}

int fmrx_carrier(fmrx_ctx* c, const float* demod, size_t n_blocks, float* sums) {
    CtxLock lock_(c);
    if (!c || !demod || !sums) return fail(FMRX_EINVAL, "null argument");
    int rc = check_frame_blocks(c, n_blocks, "a carrier call");
    if (rc || n_blocks == 0) return rc;
    if ((rc = set_device(c))) return rc;
    const size_t ns = c->cfg.n_streams, n_if = n_blocks * c->geo.if_samples;
    const size_t n_sums = ns * meter_frames(c, n_blocks) * 2;
    if ((rc = c->io.f32.ensure(ns * n_if)) || (rc = c->afc.sums.ensure(n_sums))) return rc;
    HIPCHK(hipMemcpyAsync(c->io.f32.p, demod, sizeof(float) * ns * n_if, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_carrier(c, c->io.f32.p, n_if, n_blocks, c->afc.sums.p))) return rc;
    HIPCHK(hipMemcpyAsync(sums, c->afc.sums.p, sizeof(float) * n_sums, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

int fmrx_carrier_accumulate(fmrx_carrier_report* io, const float* sums, size_t frames) {
    if (!io || (!sums && frames)) return fail(FMRX_EINVAL, "null argument");
    for (size_t f = 0; f < frames; f++) {
        io->sum += (double)sums[2 * f];
        io->sumsq += (double)sums[2 * f + 1];
    }
    io->frames += frames;
    return FMRX_OK;
}

int fmrx_afc_config_default(fmrx_afc_config* cfg) {
    if (!cfg) return fail(FMRX_EINVAL, "null argument");
    *cfg = fmrx_afc_config{1000, 1000, 50000, 16, 1, 1.0f};
    return FMRX_OK;
}

int fmrx_afc_decide(const fmrx_carrier_report* r, int bp_fs, const fmrx_afc_config* cfg, fmrx_afc_decision* out) {
    if (!r || !out) return fail(FMRX_EINVAL, "null argument");
    fmrx_afc_config def;
    (void)fmrx_afc_config_default(&def);
    if (!cfg) cfg = &def;
    if (!config_ok(*cfg)) return fail(FMRX_EINVAL, "afc: bad configuration");
    int P = 0;
    if (!meter_design(bp_fs, &P, nullptr)) return fail(FMRX_EINVAL, "afc: bp_fs %d is no positive multiple of 16000 up to %d", bp_fs, kMeterMaxP * 1000);
    if (r->frames == 0) return fail(FMRX_EINVAL, "afc: no frames in the report");
    const double n = (double)kMeterWindows * (double)P * (double)r->frames;
    const double mean = r->sum / n, ms = r->sumsq / n;
    const double two_pi = 2.0 * 3.14159265358979323846;
    const double clamped = mean < -1.0 ? -1.0 : mean > 1.0 ? 1.0 : mean;  // a NaN passes through
    const double err = std::asin(clamped) * (double)bp_fs / two_pi;
    fmrx_afc_decision d{};
    d.err_hz = err;
    d.mean = mean;
    d.mean_square = ms;
    d.carrier = ms <= (double)cfg->max_mean_square ? 1 : 0;  // a NaN: no carrier
    if (d.carrier && std::fabs(err) >= (double)cfg->deadband_hz)  // a NaN compares false: no correction
        d.correction_hz = (int32_t)((double)cfg->step_hz * std::round(err / (double)cfg->step_hz));  // round: halves away from zero
    *out = d;
    return FMRX_OK;
}

int fmrx_set_afc(fmrx_ctx* c, const fmrx_afc_config* cfg, int on) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null argument");
    fmrx_afc_config k;
    (void)fmrx_afc_config_default(&k);
    if (cfg) k = *cfg;
    if (!config_ok(k)) return fail(FMRX_EINVAL, "afc: bad configuration");
    if (on && !meter_design(c->geo.bp_fs, nullptr, nullptr)) return fail(FMRX_EINVAL, "no frame at bp_fs %d", c->geo.bp_fs);
    c->afc.cfg = k;
    c->afc.on = on != 0;
    if (on) reset_afc_reports(c);  // off: what was measured stays readable
    return FMRX_OK;
}

int fmrx_afc_get(const fmrx_ctx* c, int stream, fmrx_afc_status* out) {
    CtxLock lock_(c);
    if (!c || !out) return fail(FMRX_EINVAL, "null argument");
    if (stream < 0 || stream >= c->cfg.n_streams) return fail(FMRX_EINVAL, "stream %d of %d", stream, c->cfg.n_streams);
    const auto& a = c->afc;
    const size_t s = (size_t)stream;
    fmrx_afc_status st{};
    st.total = a.total[s];
    st.offset_hz = offsets_of(c)[s];
    st.origin_hz = a.moved ? a.origin[s] : st.offset_hz;
    st.retunes = a.retunes[s];
    st.refused = a.refused[s];
    st.decisions = a.decisions[s];
    st.last = a.last[s];
    *out = st;
    return FMRX_OK;
}

}  // extern "C"
