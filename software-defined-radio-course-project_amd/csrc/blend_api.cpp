// blend_api.cpp — soft stereo's entry points: the thresholds, the two primitives
// (blend.hip), the per-stream report, and the switch that blends every stereo stream of the calls whose
// front end writes demod rows.
#include <cmath>
#include <numeric>

#include "ctx.h"

using namespace fmrx;

namespace {

constexpr fmrx_blend_config kDefault{10.0f, 22.0f};

inline bool same_cfg(const fmrx_blend_config& a, const fmrx_blend_config& b) { return a.lo_db == b.lo_db && a.hi_db == b.hi_db; }

// meter frames of n_blocks blocks (whole granules)
inline size_t blend_frames(const fmrx_ctx* c, size_t n_blocks) {
    return n_blocks * c->geo.if_samples / ((size_t)kMeterWindows * (size_t)(c->geo.bp_fs / 1000));
}

// the thresholds of cfg (NULL: the defaults) into d, grown to hold them; the stream is drained first (a
// launch in flight may still read the old ones)
int upload_thresholds(fmrx_ctx* c, const fmrx_blend_config* cfg, DevBuf<float>& d) {
    float T[kBlendSteps];
    const fmrx_blend_config& k = cfg ? *cfg : kDefault;
    if (!blend_design(k.lo_db, k.hi_db, T))
        return fail(FMRX_EINVAL, "blend thresholds %g .. %g dB: finite, within [-20, 60], lo_db < hi_db", (double)k.lo_db, (double)k.hi_db);
    int rc = d.ensure(kBlendSteps);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(d.p, T, sizeof T, hipMemcpyHostToDevice));
    return 0;
}

// the primitives' thresholds: prim_thr holds those of the last config a primitive was given
int prim_thresholds(fmrx_ctx* c, const fmrx_blend_config* cfg) {
    const fmrx_blend_config& k = cfg ? *cfg : kDefault;
    if (c->blend.prim_thr.p && same_cfg(k, c->blend.prim_cfg)) return 0;
    const int rc = upload_thresholds(c, &k, c->blend.prim_thr);
    if (!rc) c->blend.prim_cfg = k;
    return rc;
}

// the levels kernel over d_power with a caller's carry (in and out) on the context stream
int run_levels_prim(fmrx_ctx* c, const fmrx_blend_config* cfg, const float* d_power, size_t F, float* d_carry, uint8_t* d_levels) {
    const size_t ns = c->cfg.n_streams;
    if (F < 1 || F > 0x7FFFFFFFull / kMeterTones) return fail(FMRX_EINVAL, "%zu frames: a levels call takes 1 .. %d", F, 0x7FFFFFFF / kMeterTones);
    int rc = prim_thresholds(c, cfg);
    if (rc || (rc = c->blend.prim_carry.ensure(ns * kBlendCarry))) return rc;
    BlendLevelsLaunch L{};
    L.power = d_power;
    L.frames = (int)F;
    L.thr = c->blend.prim_thr.p;
    L.carry_in = d_carry;
    L.carry_out = c->blend.prim_carry.p;  // a first lane may still read d_carry when a last one is done
    L.levels = d_levels;
    if ((rc = launch_blend_levels(L, (int)ns, c->stream))) return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "blend levels launch failed (%d)", rc);
    HIPCHK(hipMemcpyAsync(d_carry, c->blend.prim_carry.p, sizeof(float) * ns * kBlendCarry, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

}  // namespace

namespace fmrx {

bool blend_design(float lo_db, float hi_db, float* T16) {
    if (!std::isfinite(lo_db) || !std::isfinite(hi_db) || lo_db < -20.0f || hi_db > 60.0f || !(lo_db < hi_db) || !T16) return false;
    const double lo = (double)lo_db, hi = (double)hi_db;
    for (int j = 0; j < kBlendSteps; j++) T16[j] = (float)(0.5 * std::pow(10.0, (lo + (double)j * (hi - lo) / 15.0) / 10.0));
    return true;
}

void init_blend(fmrx_ctx* c) {
    // a granule without a capture rate: the fewest blocks that are whole meter frames
    const size_t frame = (size_t)kMeterWindows * (size_t)(c->geo.bp_fs / 1000);
    const size_t blocks = std::lcm((size_t)c->geo.if_samples, frame) / (size_t)c->geo.if_samples;
    c->blend.Gm = (unsigned)(blocks * c->geo.if_samples / frame);
    c->blend.A = (unsigned)(blocks * c->geo.audio_frames);
    c->blend.c = (float)(1.0 / (32.0 * (double)c->blend.A));
}

int check_blend_blocks(const fmrx_ctx* c, size_t n_blocks) {
    const size_t g = rds_granule_blocks(c);
    if (n_blocks % g != 0)
        return fail(FMRX_EINVAL, "%zu blocks: a call with soft stereo on takes whole granules of %zu blocks", n_blocks, g);
    return 0;
}

int reset_blend(fmrx_ctx* c) {
    auto& B = c->blend;
    B.rep.assign((size_t)c->cfg.n_streams, fmrx_blend_report{});  // sized here: creation resets
    B.last.assign((size_t)c->cfg.n_streams, 0);
    B.pending = 0;
    B.hold = false;
    B.carry.rewind();
    if (B.carry.cur()) HIPCHK(hipMemsetAsync(B.carry.cur(), 0, sizeof(float) * B.carry.buf[0].n, c->stream));
    return 0;
}

int refuse_blend(const fmrx_ctx* c, const char* who, const char* why) {
    return c->blend.on ? fail(FMRX_ESTATE, "%s: not with soft stereo on (%s)", who, why) : 0;
}

int blend_enqueue(fmrx_ctx* c, size_t n_blocks) {
    auto& B = c->blend;
    const size_t ns = c->cfg.n_streams, frames = blend_frames(c, n_blocks);
    B.pending = 0;
    if (B.hold) {  // every entry of a stream's row its last level; the rows go up by a blocking copy
        const size_t na = n_blocks * c->geo.audio_frames, held = (na * B.Gm + B.A - 1) / B.A;
        int rc = B.levels.ensure(ns * (held + 1));
        if (rc) return rc;
        B.hold_rows.resize(ns * (held + 1));
        for (size_t s = 0; s < ns; s++) std::fill_n(B.hold_rows.begin() + s * (held + 1), held + 1, B.last[s]);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(B.levels.p, B.hold_rows.data(), B.hold_rows.size(), hipMemcpyHostToDevice));
        B.pending = held;
        return 0;
    }
    if (frames < 1 || frames > 0x7FFFFFFFull / kMeterTones) return fail(FMRX_EINVAL, "%zu blocks: too many frames for one call", n_blocks);
    int rc = B.levels.ensure(ns * (frames + 1));
    if (rc) return rc;
    BlendLevelsLaunch L{};
    L.power = c->meter.pow.p;
    L.frames = (int)frames;
    L.thr = B.thr.p;
    L.carry_in = B.carry.cur();
    L.carry_out = B.carry.next();
    L.levels = B.levels.p;
    if ((rc = launch_blend_levels(L, (int)ns, c->stream))) return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "blend levels launch failed (%d)", rc);
    B.carry.flip();
    B.pending = frames;
    return 0;
}

int blend_apply(fmrx_ctx* c, float* rows, size_t na, bool in_place, int16_t* d_pcm) {
    const auto& B = c->blend;
    if (na > 0x7FFFFFF0ull) return fail(FMRX_EINVAL, "%zu audio frames a stream: too many for one call", na);
    BlendApplyLaunch L{};
    L.in = reinterpret_cast<const float2*>(rows);
    L.n = (unsigned)na;
    L.A = B.A;
    L.Gm = B.Gm;
    L.c = B.c;
    L.levels = B.levels.p;
    L.level_stride = B.pending + 1;
    L.out = in_place ? reinterpret_cast<float2*>(rows) : nullptr;
    L.pcm = in_place ? nullptr : d_pcm;
    const int rc = launch_blend_apply(L, c->cfg.n_streams, c->stream);
    return rc ? fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "blend apply launch failed (%d)", rc) : 0;
}

int blend_finish(fmrx_ctx* c) {
    auto& B = c->blend;
    const size_t ns = c->cfg.n_streams, frames = B.pending;
    if (frames == 0) return 0;
    B.pending = 0;
    if (B.hold) return 0;  // nothing measured, nothing counted
    B.host.resize(ns * frames);
    HIPCHK(hipMemcpy2DAsync(B.host.data(), frames, B.levels.p + 1, frames + 1, frames, ns, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t s = 0; s < ns; s++) {
        fmrx_blend_report& r = B.rep[s];
        for (size_t f = 0; f < frames; f++) r.level_frames[std::min<unsigned>(B.host[s * frames + f], kBlendSteps)]++;
        r.frames += frames;
        B.last[s] = (uint8_t)std::min<unsigned>(B.host[s * frames + frames - 1], kBlendSteps);
    }
    return 0;
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
    return fail(FMRX_EINVAL, "blend thresholds %g .. %g dB: finite, within [-20, 60], lo_db < hi_db", (double)k.lo_db, (double)k.hi_db);
}

int fmrx_blend_levels_device(fmrx_ctx* c, const fmrx_blend_config* cfg, const float* d_power, size_t F, float* d_carry,
                             uint8_t* d_levels) {
    CtxLock lock_(c);
    if (!c || !d_power || !d_carry || !d_levels) return fail(FMRX_EINVAL, "null argument");
    const int rc = set_device(c);
    return rc ? rc : run_levels_prim(c, cfg, d_power, F, d_carry, d_levels);
}

int fmrx_blend_levels(fmrx_ctx* c, const fmrx_blend_config* cfg, const float* power, size_t F, float* carry, uint8_t* levels) {
    CtxLock lock_(c);
    if (!c || !power || !carry || !levels) return fail(FMRX_EINVAL, "null argument");
    if (F < 1 || F > 0x7FFFFFFFull / kMeterTones) return fail(FMRX_EINVAL, "%zu frames: a levels call takes 1 .. %d", F, 0x7FFFFFFF / kMeterTones);
    int rc = set_device(c);
    if (rc) return rc;
    const size_t ns = c->cfg.n_streams, n_pow = ns * F * kMeterTones, n_lv = ns * (F + 1);
    // the powers, then the carry, in one buffer of floats; the level rows in the context's
    if ((rc = c->blend.prim_pow.ensure(n_pow + ns * kBlendCarry)) || (rc = c->blend.levels.ensure(n_lv))) return rc;
    float* d_carry = c->blend.prim_pow.p + n_pow;
    HIPCHK(hipMemcpyAsync(c->blend.prim_pow.p, power, sizeof(float) * n_pow, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_carry, carry, sizeof(float) * ns * kBlendCarry, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_levels_prim(c, cfg, c->blend.prim_pow.p, F, d_carry, c->blend.levels.p))) return rc;
    HIPCHK(hipMemcpyAsync(levels, c->blend.levels.p, n_lv, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(carry, d_carry, sizeof(float) * ns * kBlendCarry, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

int fmrx_blend_apply_device(fmrx_ctx* c, const float* d_rl, size_t n, const uint8_t* d_levels, float* d_out, int16_t* d_pcm) {
    CtxLock lock_(c);
    if (!c || !d_rl || !d_levels) return fail(FMRX_EINVAL, "null argument");
    if (c->cfg.channels != FMRX_STEREO) return fail(FMRX_EINVAL, "fmrx_blend_apply_device: a STEREO context's stage");
    const auto& B = c->blend;
    if (n % B.A != 0 || n > 0x7FFFFFF0ull)
        return fail(FMRX_EINVAL, "%zu audio frames: a blend call takes whole granules of %u (at most 2^31 - 16 frames)", n, B.A);
    if (n == 0) return FMRX_OK;
    if (reinterpret_cast<uintptr_t>(d_rl) % 16 != 0 || reinterpret_cast<uintptr_t>(d_out) % 16 != 0 || reinterpret_cast<uintptr_t>(d_pcm) % 4 != 0)
        return fail(FMRX_EINVAL, "fmrx_blend_apply_device: float rows 16-byte aligned, PCM rows 4-byte aligned");
    int rc = set_device(c);
    if (rc) return rc;
    BlendApplyLaunch L{};
    L.in = reinterpret_cast<const float2*>(d_rl);
    L.n = (unsigned)n;
    L.A = B.A;
    L.Gm = B.Gm;
    L.c = B.c;
    L.levels = d_levels;
    L.level_stride = n / B.A * B.Gm + 1;
    L.out = reinterpret_cast<float2*>(d_out);
    L.pcm = d_pcm;
    if ((rc = launch_blend_apply(L, c->cfg.n_streams, c->stream))) return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "blend apply launch failed (%d)", rc);
    return FMRX_OK;
}

int fmrx_set_stereo_blend(fmrx_ctx* c, int on, const fmrx_blend_config* cfg) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (c->cfg.channels != FMRX_STEREO) return fail(FMRX_EINVAL, "fmrx_set_stereo_blend: a STEREO context's stage");
    const fmrx_blend_config k = cfg ? *cfg : kDefault;
    float T[kBlendSteps];
    if (!blend_design(k.lo_db, k.hi_db, T))
        return fail(FMRX_EINVAL, "blend thresholds %g .. %g dB: finite, within [-20, 60], lo_db < hi_db", (double)k.lo_db, (double)k.hi_db);
    int rc = set_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));  // a call in flight still reads the carry and the thresholds
    auto& B = c->blend;
    if (on) {  // everything but a call's rows now, so that a blended call allocates nothing else
        if ((rc = B.carry.ensure((size_t)c->cfg.n_streams * kBlendCarry)) || (rc = upload_thresholds(c, &k, B.thr))) return rc;
        // the meter's tables too: fmrx_set_meter's own path (its switch is put back as it was)
        const bool meter_on = c->meter.on;
        if ((rc = fmrx_set_meter(c, 1))) return rc;
        c->meter.on = meter_on;
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
    c->blend.hold = on != 0;
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
