// meter_api.cpp — the subcarrier meter's entry points: the tables, the primitive over
// demod rows (meter.hip), the host-side report and decision, and the switch that runs the meter inside
// the calls whose front end writes demod rows.
#include <cmath>
#include <numeric>

#include "ctx.h"

using namespace fmrx;

namespace {

constexpr int kToneKHz[kMeterTones] = {17, 19, 21, 56, 58, 61, 63};
constexpr double kPowerFloor = 1e-30;  // below it a sum counts as this (no log of zero)

// the tables on the device, once a context
int ensure_meter_tables(fmrx_ctx* c) {
    if (c->meter.p) return 0;
    int P = 0;
    if (!meter_design(c->geo.bp_fs, &P, nullptr)) return fail(FMRX_EINVAL, "no meter design at bp_fs %d", c->geo.bp_fs);
    std::vector<float> tab((size_t)2 * kMeterTones * (size_t)P);
    meter_design(c->geo.bp_fs, nullptr, tab.data());
    int rc = c->meter.tab.ensure(tab.size());
    if (rc) return rc;
    HIPCHK(hipMemcpy(c->meter.tab.p, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    c->meter.p = P;
    return 0;
}

// the kernel over the rows at d_demod (whole frames) into d_power, enqueued
int run_meter(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_blocks, float* d_power) {
    int rc = ensure_meter_tables(c);
    if (rc) return rc;
    const size_t frames = meter_frames(c, n_blocks);
    if (frames > 0x7FFFFFFFull) return fail(FMRX_EINVAL, "%zu blocks: too many frames for one meter call", n_blocks);
    MeterLaunch L{};
    L.demod = d_demod;
    L.demod_stride = demod_stride;
    L.tables = c->meter.tab.p;
    L.P = c->meter.p;
    L.frames = (int)frames;
    L.power = d_power;
    return (rc = launch_meter(L, c->cfg.n_streams, c->stream)) ? launch_failed(rc, "meter") : 0;
}

inline double db10(double x) { return 10.0 * std::log10(x); }

}  // namespace

namespace fmrx {

bool meter_design(int bp_fs, int* P, float* tables) {
    if (bp_fs <= 0 || bp_fs % 16000 != 0 || bp_fs / 1000 > kMeterMaxP) return false;
    const int p = bp_fs / 1000;
    if (P) *P = p;
    if (!tables) return true;
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int t = 0; t < kMeterTones; t++)
        for (int n = 0; n < p; n++) {
            const double w = 0.5 - 0.5 * std::cos(two_pi * (double)n / (double)p);
            const double a = two_pi * (double)((kToneKHz[t] * n) % p) / (double)p;
            tables[(size_t)(2 * t) * p + n] = (float)(w * std::cos(a));
            tables[(size_t)(2 * t + 1) * p + n] = (float)(w * std::sin(a));
        }
    return true;
}

void init_frames(fmrx_ctx* c) {
    // a granule without a capture rate: the fewest blocks that are whole meter frames
    const size_t frame = (size_t)kMeterWindows * (size_t)(c->geo.bp_fs / 1000);
    const size_t blocks = std::lcm((size_t)c->geo.if_samples, frame) / (size_t)c->geo.if_samples;
    c->frames.Gm = (unsigned)(blocks * c->geo.if_samples / frame);
    c->frames.A = (unsigned)(blocks * c->geo.audio_frames);
}

int check_frame_blocks(const fmrx_ctx* c, size_t n_blocks, const char* who) {
    const size_t g = rds_granule_blocks(c);  // a frame is the RDS window: 64 ms
    if (n_blocks % g != 0)
        return fail(FMRX_EINVAL, "%zu blocks: %s takes whole frames, granules of %zu blocks", n_blocks, who, g);
    return 0;
}

int meter_tables_ready(fmrx_ctx* c) {
    const bool on = c->meter.on;
    const int rc = fmrx_set_meter(c, 1);
    c->meter.on = on;
    return rc;
}

void reset_meter(fmrx_ctx* c) {
    c->meter.rep.assign((size_t)c->cfg.n_streams, fmrx_meter_report{});  // sized here: creation resets
    c->meter.pending = 0;
}

int meter_enqueue(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_blocks) {
    const size_t ns = c->cfg.n_streams, frames = meter_frames(c, n_blocks);
    c->meter.pending = 0;
    int rc;
    if ((rc = c->meter.pow.ensure(ns * frames * kMeterTones))) return rc;
    if ((rc = run_meter(c, d_demod, demod_stride, n_blocks, c->meter.pow.p))) return rc;
    c->meter.pending = frames;
    return 0;
}

int meter_finish(fmrx_ctx* c) {
    const size_t ns = c->cfg.n_streams, frames = c->meter.pending;
    if (frames == 0) return 0;
    c->meter.pending = 0;
    c->meter.host.resize(ns * frames * kMeterTones);
    HIPCHK(hipMemcpyAsync(c->meter.host.data(), c->meter.pow.p, sizeof(float) * c->meter.host.size(), hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t s = 0; s < ns; s++) {
        int rc = fmrx_meter_accumulate(&c->meter.rep[s], c->meter.host.data() + s * frames * kMeterTones, frames);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace fmrx

extern "C" {

int fmrx_meter_design(int bp_fs, int* P, float* tables) {
    if (meter_design(bp_fs, P, tables)) return FMRX_OK;
    return fail(FMRX_EINVAL, "meter: bp_fs %d is no positive multiple of 16000 up to %d", bp_fs, kMeterMaxP * 1000);
}

int fmrx_meter_device(fmrx_ctx* c, const float* d_demod, size_t n_blocks, float* d_power) {
    CtxLock lock_(c);
    if (!c || !d_demod || !d_power) return fail(FMRX_EINVAL, "null argument");
    int rc = check_frame_blocks(c, n_blocks, "a meter call");
    if (rc || n_blocks == 0) return rc;
    if ((rc = set_device(c))) return rc;
    return run_meter(c, d_demod, n_blocks * c->geo.if_samples, n_blocks, d_power);
}

int fmrx_meter(fmrx_ctx* c, const float* demod, size_t n_blocks, float* power) {
    CtxLock lock_(c);
    if (!c || !demod || !power) return fail(FMRX_EINVAL, "null argument");
    int rc = check_frame_blocks(c, n_blocks, "a meter call");
    if (rc || n_blocks == 0) return rc;
    if ((rc = set_device(c))) return rc;
    const size_t ns = c->cfg.n_streams, n_if = n_blocks * c->geo.if_samples;
    const size_t n_pow = ns * meter_frames(c, n_blocks) * kMeterTones;
    if ((rc = c->io.f32.ensure(ns * n_if)) || (rc = c->meter.pow.ensure(n_pow))) return rc;
    HIPCHK(hipMemcpyAsync(c->io.f32.p, demod, sizeof(float) * ns * n_if, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_meter(c, c->io.f32.p, n_if, n_blocks, c->meter.pow.p))) return rc;
    HIPCHK(hipMemcpyAsync(power, c->meter.pow.p, sizeof(float) * n_pow, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

int fmrx_meter_config_default(fmrx_meter_config* cfg) {
    if (!cfg) return fail(FMRX_EINVAL, "null argument");
    cfg->pilot_min_snr_db = 10.0f;
    cfg->rds_min_snr_db = 1.94f;
    return FMRX_OK;
}

int fmrx_meter_accumulate(fmrx_meter_report* io, const float* power, size_t frames) {
    if (!io || (!power && frames)) return fail(FMRX_EINVAL, "null argument");
    for (size_t f = 0; f < frames; f++)
        for (int t = 0; t < kMeterTones; t++) io->sum[t] += (double)power[f * kMeterTones + t];
    io->frames += frames;
    return FMRX_OK;
}

int fmrx_meter_detect(const fmrx_meter_report* r, const fmrx_meter_config* cfg, fmrx_subcarriers* out) {
    if (!r || !out) return fail(FMRX_EINVAL, "null argument");
    if (r->frames == 0) return fail(FMRX_EINVAL, "meter: no frames in the report");
    fmrx_meter_config def;
    (void)fmrx_meter_config_default(&def);
    if (!cfg) cfg = &def;
    const double windows = (double)kMeterWindows * (double)r->frames;
    const double pilot = std::max(r->sum[1], kPowerFloor), guard = std::max((r->sum[0] + r->sum[2]) / 2.0, kPowerFloor);
    const double side = std::max((r->sum[3] + r->sum[4]) / 2.0, kPowerFloor);
    const double above = std::max((r->sum[5] + r->sum[6]) / 2.0, kPowerFloor);
    const double pilot_snr = db10(pilot / guard), rds_snr = db10(side / above);
    out->pilot_db = (float)db10(pilot / windows);
    out->pilot_snr_db = (float)pilot_snr;
    out->rds_db = (float)db10(side / windows);
    out->rds_snr_db = (float)rds_snr;
    out->stereo = pilot_snr >= (double)cfg->pilot_min_snr_db ? 1 : 0;
    out->rds = rds_snr >= (double)cfg->rds_min_snr_db ? 1 : 0;
    return FMRX_OK;
}

int fmrx_set_meter(fmrx_ctx* c, int on) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null argument");
    if (on) {  // the tables now, so that a metered call allocates nothing but its powers
        int rc = set_device(c);
        if (rc || (rc = ensure_meter_tables(c))) return rc;
    }
    c->meter.on = on != 0;
    return FMRX_OK;
}

int fmrx_meter_get(const fmrx_ctx* c, int stream, fmrx_meter_report* out) {
    CtxLock lock_(c);
    if (!c || !out) return fail(FMRX_EINVAL, "null argument");
    if (stream < 0 || stream >= c->cfg.n_streams) return fail(FMRX_EINVAL, "stream %d of %d", stream, c->cfg.n_streams);
    *out = c->meter.rep[(size_t)stream];
    return FMRX_OK;
}

}  // extern "C"
