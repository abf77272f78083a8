// blend_api.cpp — soft stereo's entry points: the thresholds, the two primitives
// (blend.hip), the per-stream report, and the switch that blends every stereo stream of the calls whose
// front end writes demod rows.
#include <cmath>

#include "ctx.h"

using namespace fmrx;

namespace {

constexpr fmrx_blend_config kDefault{10.0f, 22.0f};

inline bool same_cfg(const fmrx_blend_config& a, const fmrx_blend_config& b) { return a.lo_db == b.lo_db && a.hi_db == b.hi_db; }

constexpr const char* kBadCfg = "blend thresholds %g .. %g dB: finite, within [-20, 60], lo_db < hi_db";

// the primitives' thresholds: f.prim_thr holds those of the last config a primitive was given
int prim_thresholds(fmrx_ctx* c, const fmrx_blend_config* cfg) {
    auto& B = c->blend;
    const fmrx_blend_config& k = cfg ? *cfg : kDefault;
    if (B.f.prim_thr.p && same_cfg(k, B.prim_cfg)) return 0;
    float T[kBlendSteps];
    if (!blend_design(k.lo_db, k.hi_db, T)) return fail(FMRX_EINVAL, kBadCfg, (double)k.lo_db, (double)k.hi_db);
    const int rc = upload_floats(c, T, kBlendSteps, B.f.prim_thr);
    if (!rc) B.prim_cfg = k;
    return rc;
}

// one stream's level bytes of a call into its report (levels_finish's count)
void count_row(void* reports, size_t stream, const uint8_t* row, size_t frames) {
    fmrx_blend_report& r = static_cast<fmrx_blend_report*>(reports)[stream];
    for (size_t f = 0; f < frames; f++) r.level_frames[row[f]]++;
    r.frames += frames;
}

// the launch of n frames a stream by the rows of `levels`; out and pcm are the caller's
int run_apply(fmrx_ctx* c, const float* rows, size_t n, const uint8_t* d_levels, size_t level_stride, float* d_out, int16_t* d_pcm) {
    BlendApplyLaunch L{};
    L.in = reinterpret_cast<const float2*>(rows);
    L.n = (unsigned)n;
    L.A = c->frames.A;
    L.Gm = c->frames.Gm;
    L.c = c->blend.c;
    L.levels = d_levels;
    L.level_stride = level_stride;
    L.out = reinterpret_cast<float2*>(d_out);
    L.pcm = d_pcm;
    const int rc = launch_blend_apply(L, c->cfg.n_streams, c->stream);
    return rc ? launch_failed(rc, "blend apply") : 0;
}

}  // namespace

namespace fmrx {

bool blend_design(float lo_db, float hi_db, float* T16) {
    if (!std::isfinite(lo_db) || !std::isfinite(hi_db) || lo_db < -20.0f || hi_db > 60.0f || !(lo_db < hi_db) || !T16) return false;
    const double lo = (double)lo_db, hi = (double)hi_db;
    for (int j = 0; j < kBlendSteps; j++) T16[j] = (float)(0.5 * std::pow(10.0, (lo + (double)j * (hi - lo) / 15.0) / 10.0));
    return true;
}

void init_blend(fmrx_ctx* c) { c->blend.c = (float)(1.0 / (32.0 * (double)c->frames.A)); }

int reset_blend(fmrx_ctx* c) {
    c->blend.rep.assign((size_t)c->cfg.n_streams, fmrx_blend_report{});  // sized here: creation resets
    return levels_reset(c->blend.f, c->stream, (size_t)c->cfg.n_streams);
}

int blend_apply(fmrx_ctx* c, float* rows, size_t na, bool in_place, int16_t* d_pcm) {
    if (na > 0x7FFFFFF0ull) return fail(FMRX_EINVAL, "%zu audio frames a stream: too many for one call", na);
    return run_apply(c, rows, na, c->blend.f.levels.p, c->blend.f.stride(), in_place ? rows : nullptr, in_place ? nullptr : d_pcm);
}

int blend_finish(fmrx_ctx* c) {
    return levels_finish(c->blend.f, c->stream, (size_t)c->cfg.n_streams, count_row, c->blend.rep.data());
}

}  // namespace fmrx

extern "C" {

int fmrx_blend_config_default(fmrx_blend_config* cfg) {
    if (!cfg) return fail(FMRX_EINVAL, "null argument");
    *cfg = kDefault;
    return FMRX_OK;
}

int fmrx_blend_design(const fmrx_blend_config* cfg, float* T16) {
    if (!T16) return fail(FMRX_EINVAL, "null argument");
    const fmrx_blend_config& k = cfg ? *cfg : kDefault;
    if (blend_design(k.lo_db, k.hi_db, T16)) return FMRX_OK;
    return fail(FMRX_EINVAL, kBadCfg, (double)k.lo_db, (double)k.hi_db);
}

int fmrx_blend_levels_device(fmrx_ctx* c, const fmrx_blend_config* cfg, const float* d_power, size_t F, float* d_carry,
                             uint8_t* d_levels) {
    CtxLock lock_(c);
    if (!c || !d_power || !d_carry || !d_levels) return fail(FMRX_EINVAL, "null argument");
    const int rc = set_device(c);
    return rc ? rc : levels_prim_device(c->blend.f, c->stream, (size_t)c->cfg.n_streams, [&] { return prim_thresholds(c, cfg); }, d_power, F, d_carry, d_levels);
}

int fmrx_blend_levels(fmrx_ctx* c, const fmrx_blend_config* cfg, const float* power, size_t F, float* carry, uint8_t* levels) {
    CtxLock lock_(c);
    if (!c || !power || !carry || !levels) return fail(FMRX_EINVAL, "null argument");
    int rc = levels_check_frames(F);
    if (rc || (rc = set_device(c))) return rc;
    return levels_prim_host(c->blend.f, c->stream, (size_t)c->cfg.n_streams, [&] { return prim_thresholds(c, cfg); }, power, F, carry, levels);
}

int fmrx_blend_apply_device(fmrx_ctx* c, const float* d_rl, size_t n, const uint8_t* d_levels, float* d_out, int16_t* d_pcm) {
    CtxLock lock_(c);
    if (!c || !d_rl || !d_levels) return fail(FMRX_EINVAL, "null argument");
    if (c->cfg.channels != FMRX_STEREO) return fail(FMRX_EINVAL, "fmrx_blend_apply_device: a STEREO context's stage");
    const unsigned A = c->frames.A;
    if (n % A != 0 || n > 0x7FFFFFF0ull)
        return fail(FMRX_EINVAL, "%zu audio frames: a blend call takes whole granules of %u (at most 2^31 - 16 frames)", n, A);
    if (n == 0) return FMRX_OK;
    if (reinterpret_cast<uintptr_t>(d_rl) % 16 != 0 || reinterpret_cast<uintptr_t>(d_out) % 16 != 0 || reinterpret_cast<uintptr_t>(d_pcm) % 4 != 0)
        return fail(FMRX_EINVAL, "fmrx_blend_apply_device: float rows 16-byte aligned, PCM rows 4-byte aligned");
    const int rc = set_device(c);
    return rc ? rc : run_apply(c, d_rl, n, d_levels, level_row_bytes(1, n / A * c->frames.Gm), d_out, d_pcm);
}

int fmrx_set_stereo_blend(fmrx_ctx* c, int on, const fmrx_blend_config* cfg) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (c->cfg.channels != FMRX_STEREO) return fail(FMRX_EINVAL, "fmrx_set_stereo_blend: a STEREO context's stage");
    const fmrx_blend_config k = cfg ? *cfg : kDefault;
    float T[kBlendSteps];
    if (!blend_design(k.lo_db, k.hi_db, T)) return fail(FMRX_EINVAL, kBadCfg, (double)k.lo_db, (double)k.hi_db);
    int rc = set_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));  // a call in flight still reads the carry and the thresholds
    auto& B = c->blend;
    if (on) {  // everything but a call's rows now, so that a blended call allocates nothing else
        if ((rc = B.f.carry.ensure((size_t)c->cfg.n_streams * kLevelCarry)) || (rc = upload_floats(c, T, kBlendSteps, B.thr)) ||
            (rc = meter_tables_ready(c)))
            return rc;
    }
    B.cfg = k;
    B.on = on != 0;
    if ((rc = reset_blend(c))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

int fmrx_blend_hold(fmrx_ctx* c, int on) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (on && !c->blend.on) return fail(FMRX_ESTATE, "fmrx_blend_hold: soft stereo is off (fmrx_set_stereo_blend first)");
    c->blend.f.hold = on != 0;
    return FMRX_OK;
}

int fmrx_stereo_blend(const fmrx_ctx* c, int* on, fmrx_blend_config* cfg) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (on) *on = c->blend.on ? 1 : 0;
    if (cfg) *cfg = c->blend.cfg;
    return FMRX_OK;
}

int fmrx_blend_get(const fmrx_ctx* c, int stream, fmrx_blend_report* out) {
    CtxLock lock_(c);
    if (!c || !out) return fail(FMRX_EINVAL, "null argument");
    if (stream < 0 || stream >= c->cfg.n_streams) return fail(FMRX_EINVAL, "stream %d of %d", stream, c->cfg.n_streams);
    *out = c->blend.rep[(size_t)stream];
    return FMRX_OK;
}

}  // extern "C"
