// quiet_api.cpp — quieting's entry points: the design, the two primitives (quiet.hip), the
// per-stream report, and the switch that rolls off and turns down every stream of the calls whose front
// end writes demod rows.
#include <cmath>

#include "ctx.h"

using namespace fmrx;

namespace {

constexpr fmrx_quiet_config kDefault{22.0f, 34.0f, 36.0f, 44.0f, 20.0f, 2500};
constexpr double kPi = 3.14159265358979323846;
constexpr int kTabFloats = 2 * kQuietSteps + kQuietTaps;  // Tc, Tm, the taps
constexpr const char* kBadCfg =
    "quieting config: every float finite, cut_lo_db < cut_hi_db and mute_lo_db < mute_hi_db within [-40, 80], mute_depth_db "
    "in [0, 60], corner_hz at most 8000 and high enough for 64 taps (2069 Hz at 48 kHz, 1901 Hz at 44.1 kHz)";

struct Design {
    float tab[kTabFloats];
    float g0, cg, cw;
};

inline bool same_cfg(const fmrx_quiet_config& a, const fmrx_quiet_config& b) {
    return a.cut_lo_db == b.cut_lo_db && a.cut_hi_db == b.cut_hi_db && a.mute_lo_db == b.mute_lo_db && a.mute_hi_db == b.mute_hi_db &&
           a.mute_depth_db == b.mute_depth_db && a.corner_hz == b.corner_hz;
}

// audio frames a granule at the audio rates the modes have (0: none of them)
inline unsigned granule_frames(int audio_fs) { return audio_fs == 48000 ? 3072u : audio_fs == 44100 ? 56448u : 0u; }

inline bool bounds_ok(float lo, float hi) {
    return std::isfinite(lo) && std::isfinite(hi) && lo >= -40.0f && hi <= 80.0f && lo < hi;
}

// fmrx_quiet_design: false, nothing written, for a rate or a config outside the definition
bool quiet_design(int audio_fs, int bp_fs, const fmrx_quiet_config& k, Design* d) {
    int P = 0;
    const unsigned A = granule_frames(audio_fs);
    if (A == 0 || !meter_design(bp_fs, &P, nullptr)) return false;
    if (!bounds_ok(k.cut_lo_db, k.cut_hi_db) || !bounds_ok(k.mute_lo_db, k.mute_hi_db)) return false;
    if (!std::isfinite(k.mute_depth_db) || k.mute_depth_db < 0.0f || k.mute_depth_db > 60.0f) return false;
    if (k.corner_hz > 8000 || !(std::exp(-128.0 * kPi * (double)k.corner_hz / (double)audio_fs) < std::ldexp(1.0, -25))) return false;
    const double scale = 4.0 * ((double)P / 240.0);
    const double bounds[2][2] = {{(double)k.cut_lo_db, (double)k.cut_hi_db}, {(double)k.mute_lo_db, (double)k.mute_hi_db}};
    for (int b = 0; b < 2; b++)
        for (int j = 0; j < kQuietSteps; j++) {
            const double lo = bounds[b][0], hi = bounds[b][1];
            d->tab[b * kQuietSteps + j] = (float)(scale * std::pow(10.0, (hi - (double)j * (hi - lo) / 15.0) / 10.0));
        }
    const double p = std::exp(-2.0 * kPi * (double)k.corner_hz / (double)audio_fs);
    double r = 1.0 - p;
    for (int n = 0; n < kQuietTaps; n++) {
        d->tab[2 * kQuietSteps + n] = (float)r;
        r = r * p;
    }
    d->g0 = (float)std::pow(10.0, -(double)k.mute_depth_db / 20.0);
    d->cg = (float)((1.0 - (double)d->g0) / (16.0 * (double)A));
    d->cw = (float)(1.0 / (16.0 * (double)A));
    return true;
}

inline bool ctx_design(const fmrx_ctx* c, const fmrx_quiet_config& k, Design* d) {
    return quiet_design(deemph_audio_fs(c), c->geo.bp_fs, k, d) && granule_frames(deemph_audio_fs(c)) == c->frames.A;
}

// the context's thresholds, taps and gains on the device, once a config
int ensure_tab(fmrx_ctx* c) {
    auto& Q = c->quiet;
    if (Q.tab.p) return 0;
    Design d;
    if (!ctx_design(c, Q.cfg, &d)) return fail(FMRX_EINVAL, "%s", kBadCfg);
    const int rc = upload_floats(c, d.tab, kTabFloats, Q.tab);
    if (!rc) Q.g0 = d.g0, Q.cg = d.cg, Q.cw = d.cw;
    return rc;
}

// the levels primitive's thresholds: f.prim_thr holds those of the last config it was given
int prim_thresholds(fmrx_ctx* c, const fmrx_quiet_config* cfg) {
    auto& Q = c->quiet;
    const fmrx_quiet_config& k = cfg ? *cfg : kDefault;
    if (Q.f.prim_thr.p && same_cfg(k, Q.prim_cfg)) return 0;
    Design d;
    if (!ctx_design(c, k, &d)) return fail(FMRX_EINVAL, "%s", kBadCfg);
    const int rc = upload_floats(c, d.tab, 2 * kQuietSteps, Q.f.prim_thr);
    if (!rc) Q.prim_cfg = k;
    return rc;
}

// one stream's level pairs (c, m) of a call into its report (levels_finish's count)
void count_row(void* reports, size_t stream, const uint8_t* row, size_t frames) {
    fmrx_quiet_report& r = static_cast<fmrx_quiet_report*>(reports)[stream];
    for (size_t f = 0; f < frames; f++) {
        r.cut_frames[row[2 * f]]++;
        r.mute_frames[row[2 * f + 1]]++;
    }
    r.frames += frames;
}

// the launch of na frames a stream with the context's taps and gains; levels, history and outlets are the caller's
QuietApplyLaunch apply_launch(const fmrx_ctx* c, const float* rows, size_t na) {
    const auto& Q = c->quiet;
    QuietApplyLaunch L{};
    L.in = rows;
    L.nch = c->cfg.channels == FMRX_MONO ? 1 : 2;
    L.stride = na * (size_t)L.nch;
    L.n = (unsigned)na;
    L.A = c->frames.A;
    L.Gm = c->frames.Gm;
    L.g0 = Q.g0;
    L.cg = Q.cg;
    L.cw = Q.cw;
    L.h = Q.tab.p + 2 * kQuietSteps;
    return L;
}

}  // namespace

namespace fmrx {

int reset_quiet(fmrx_ctx* c) {
    auto& Q = c->quiet;
    Q.rep.assign((size_t)c->cfg.n_streams, fmrx_quiet_report{});  // sized here: creation resets
    Q.hist.rewind();
    const int rc = levels_reset(Q.f, c->stream, (size_t)c->cfg.n_streams);
    if (!rc && Q.hist.cur()) HIPCHK(hipMemsetAsync(Q.hist.cur(), 0, sizeof(float) * Q.hist.buf[0].n, c->stream));
    return rc;
}

int quiet_apply(fmrx_ctx* c, const float* rows, size_t na, float* d_out, int16_t* d_pcm) {
    auto& Q = c->quiet;
    if (na > 0x7FFFFFF0ull) return fail(FMRX_EINVAL, "%zu audio frames a stream: too many for one call", na);
    QuietApplyLaunch L = apply_launch(c, rows, na);
    L.levels = Q.f.levels.p;
    L.level_stride = Q.f.stride();
    L.state_in = Q.hist.cur();
    L.state_out = Q.hist.next();
    L.out = d_out;
    L.pcm = d_pcm;
    const int rc = launch_quiet_apply(L, c->cfg.n_streams, c->stream);
    if (rc) return launch_failed(rc, "quieting apply");
    Q.hist.flip();
    return 0;
}

int quiet_finish(fmrx_ctx* c) {
    return levels_finish(c->quiet.f, c->stream, (size_t)c->cfg.n_streams, count_row, c->quiet.rep.data());
}

}  // namespace fmrx

extern "C" {

int fmrx_quiet_config_default(fmrx_quiet_config* cfg) {
    if (!cfg) return fail(FMRX_EINVAL, "null argument");
    *cfg = kDefault;
    return FMRX_OK;
}

int fmrx_quiet_design(int audio_fs, int bp_fs, const fmrx_quiet_config* cfg, float* Tc16, float* Tm16, float* h64, float* g0_cg_cw) {
    Design d;
    if (!quiet_design(audio_fs, bp_fs, cfg ? *cfg : kDefault, &d))
        return fail(FMRX_EINVAL, "audio_fs %d (48000 or 44100), bp_fs %d (as fmrx_meter_design takes it); %s", audio_fs, bp_fs, kBadCfg);
    if (Tc16) std::copy_n(d.tab, kQuietSteps, Tc16);
    if (Tm16) std::copy_n(d.tab + kQuietSteps, kQuietSteps, Tm16);
    if (h64) std::copy_n(d.tab + 2 * kQuietSteps, kQuietTaps, h64);
    if (g0_cg_cw) g0_cg_cw[0] = d.g0, g0_cg_cw[1] = d.cg, g0_cg_cw[2] = d.cw;
    return FMRX_OK;
}

int fmrx_quiet_levels_device(fmrx_ctx* c, const fmrx_quiet_config* cfg, const float* d_power, size_t F, float* d_carry,
                             uint8_t* d_levels) {
    CtxLock lock_(c);
    if (!c || !d_power || !d_carry || !d_levels) return fail(FMRX_EINVAL, "null argument");
    const int rc = set_device(c);
    return rc ? rc : levels_prim_device(c->quiet.f, c->stream, (size_t)c->cfg.n_streams, [&] { return prim_thresholds(c, cfg); }, d_power, F, d_carry, d_levels);
}

int fmrx_quiet_levels(fmrx_ctx* c, const fmrx_quiet_config* cfg, const float* power, size_t F, float* carry, uint8_t* levels) {
    CtxLock lock_(c);
    if (!c || !power || !carry || !levels) return fail(FMRX_EINVAL, "null argument");
    int rc = levels_check_frames(F);
    if (rc || (rc = set_device(c))) return rc;
    return levels_prim_host(c->quiet.f, c->stream, (size_t)c->cfg.n_streams, [&] { return prim_thresholds(c, cfg); }, power, F, carry, levels);
}

int fmrx_quiet_apply_device(fmrx_ctx* c, const float* d_in, size_t n, const uint8_t* d_levels, float* d_state, float* d_out,
                            int16_t* d_pcm) {
    CtxLock lock_(c);
    if (!c || !d_in || !d_levels || !d_state || (!d_out && !d_pcm)) return fail(FMRX_EINVAL, "null argument");
    const unsigned A = c->frames.A, Gm = c->frames.Gm;
    if (n % A != 0 || n > 0x7FFFFFF0ull)
        return fail(FMRX_EINVAL, "%zu audio frames: a quieting call takes whole granules of %u (at most 2^31 - 16 frames)", n, A);
    const size_t ns = c->cfg.n_streams, nch = c->cfg.channels == FMRX_MONO ? 1 : 2, total = ns * n * nch;
    if (d_out && d_out < d_in + total && d_in < d_out + total)
        return fail(FMRX_EINVAL, "fmrx_quiet_apply_device: not in place (d_out overlaps d_in)");
    if (reinterpret_cast<uintptr_t>(d_in) % 4 != 0 || reinterpret_cast<uintptr_t>(d_out) % 4 != 0 || reinterpret_cast<uintptr_t>(d_pcm) % 2 != 0)
        return fail(FMRX_EINVAL, "fmrx_quiet_apply_device: misaligned rows");
    if (n == 0) return FMRX_OK;
    int rc = set_device(c);
    if (rc || (rc = ensure_tab(c)) || (rc = c->quiet.prim_hist.ensure(ns * nch * kQuietHist))) return rc;
    QuietApplyLaunch L = apply_launch(c, d_in, n);
    L.levels = d_levels;
    L.level_stride = level_row_bytes(2, n / A * Gm);
    L.state_in = d_state;
    L.state_out = c->quiet.prim_hist.p;  // a first workgroup may still read d_state when a last one is done
    L.out = d_out;
    L.pcm = d_pcm;
    if ((rc = launch_quiet_apply(L, (int)ns, c->stream))) return launch_failed(rc, "quieting apply");
    HIPCHK(hipMemcpyAsync(d_state, c->quiet.prim_hist.p, sizeof(float) * ns * nch * kQuietHist, hipMemcpyDeviceToDevice, c->stream));
    return FMRX_OK;
}

int fmrx_set_quieting(fmrx_ctx* c, int on, const fmrx_quiet_config* cfg) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    const fmrx_quiet_config k = cfg ? *cfg : kDefault;
    Design d;
    if (!ctx_design(c, k, &d)) return fail(FMRX_EINVAL, "%s", kBadCfg);
    int rc = set_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));  // a call in flight still reads the carries and the tables
    auto& Q = c->quiet;
    const size_t ns = c->cfg.n_streams, rows = ns * (size_t)c->cfg.channels;
    if (on) {  // everything but a call's rows now, so that a quieted call allocates nothing else
        if ((rc = Q.f.carry.ensure(ns * kLevelCarry)) || (rc = Q.hist.ensure(rows * kQuietHist)) || (rc = meter_tables_ready(c))) return rc;
    }
    if ((on || Q.tab.p) && (rc = upload_floats(c, d.tab, kTabFloats, Q.tab))) return rc;  // (else: at a primitive's first run)
    Q.g0 = d.g0, Q.cg = d.cg, Q.cw = d.cw;
    Q.cfg = k;
    Q.on = on != 0;
    if ((rc = reset_quiet(c))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

int fmrx_quiet_hold(fmrx_ctx* c, int on) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (on && !c->quiet.on) return fail(FMRX_ESTATE, "fmrx_quiet_hold: quieting is off (fmrx_set_quieting first)");
    c->quiet.f.hold = on != 0;
    return FMRX_OK;
}

int fmrx_quieting(const fmrx_ctx* c, int* on, fmrx_quiet_config* cfg) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (on) *on = c->quiet.on ? 1 : 0;
    if (cfg) *cfg = c->quiet.cfg;
    return FMRX_OK;
}

int fmrx_quiet_get(const fmrx_ctx* c, int stream, fmrx_quiet_report* out) {
    CtxLock lock_(c);
    if (!c || !out) return fail(FMRX_EINVAL, "null argument");
    if (stream < 0 || stream >= c->cfg.n_streams) return fail(FMRX_EINVAL, "stream %d of %d", stream, c->cfg.n_streams);
    *out = c->quiet.rep[(size_t)stream];
    return FMRX_OK;
}

}  // extern "C"
