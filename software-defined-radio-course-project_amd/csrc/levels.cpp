// levels.cpp — the level follower's code (levels.h): the one place with the level rows' stride arithmetic.
#include "ctx.h"

namespace fmrx {

int levels_reset(LevelFollower& F, hipStream_t st, size_t ns) {
    F.last.assign(ns * (size_t)F.K, 0);
    F.pending = 0;
    F.hold = false;
    F.carry.rewind();
    if (F.carry.cur()) HIPCHK(hipMemsetAsync(F.carry.cur(), 0, sizeof(float) * F.carry.buf[0].n, st));
    return 0;
}

int levels_enqueue(LevelFollower& F, hipStream_t st, size_t ns, const float* d_power, const float* d_thr, size_t frames) {
    F.pending = 0;
    int rc = F.levels.ensure(ns * level_row_bytes(F.K, frames));
    if (rc) return rc;
    LevelsLaunch L{};
    L.power = d_power;
    L.frames = (int)frames;
    L.thr = d_thr;
    L.carry_in = F.carry.cur();
    L.carry_out = F.carry.next();
    L.levels = F.levels.p;
    if ((rc = F.launch(L, (int)ns, st))) return launch_failed(rc, F.what);
    F.carry.flip();
    F.pending = frames;
    return 0;
}

int levels_enqueue_held(LevelFollower& F, hipStream_t st, size_t ns, size_t held) {
    const size_t K = (size_t)F.K, row = level_row_bytes(F.K, held);
    F.pending = 0;
    int rc = F.levels.ensure(ns * row);
    if (rc) return rc;
    F.hold_rows.resize(ns * row);
    for (size_t s = 0; s < ns; s++)
        for (size_t b = 0; b < row; b++) F.hold_rows[s * row + b] = F.last[K * s + b % K];
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(F.levels.p, F.hold_rows.data(), F.hold_rows.size(), hipMemcpyHostToDevice));
    F.pending = held;
    return 0;
}

int levels_finish(LevelFollower& F, hipStream_t st, size_t ns, LevelFollower::CountRow count, void* reports) {
    const size_t K = (size_t)F.K, frames = F.pending, row = K * frames;
    if (frames == 0) return 0;
    F.pending = 0;
    if (F.hold) return 0;  // nothing measured, nothing counted
    F.host.resize(ns * row);
    HIPCHK(hipMemcpy2DAsync(F.host.data(), row, F.levels.p + K, level_row_bytes(F.K, frames), row, ns, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint8_t& b : F.host) b = (uint8_t)std::min<unsigned>(b, kLevelMax);
    for (size_t s = 0; s < ns; s++) {
        const uint8_t* r = F.host.data() + s * row;
        count(reports, s, r, frames);
        std::copy_n(r + row - K, K, F.last.begin() + K * s);
    }
    return 0;
}

int levels_check_frames(size_t frames) {
    if (frames < 1 || frames > 0x7FFFFFFFull / kMeterTones)
        return fail(FMRX_EINVAL, "%zu frames: a levels call takes 1 .. %d", frames, 0x7FFFFFFF / kMeterTones);
    return 0;
}

int levels_prim_device(LevelFollower& F, hipStream_t st, size_t ns, const std::function<int()>& thresholds, const float* d_power,
                       size_t frames, float* d_carry, uint8_t* d_levels) {
    int rc = levels_check_frames(frames);
    if (rc || (rc = thresholds()) || (rc = F.prim_carry.ensure(ns * kLevelCarry))) return rc;
    LevelsLaunch L{};
    L.power = d_power;
    L.frames = (int)frames;
    L.thr = F.prim_thr.p;
    L.carry_in = d_carry;
    L.carry_out = F.prim_carry.p;  // a first lane may still read d_carry when a last one is done
    L.levels = d_levels;
    if ((rc = F.launch(L, (int)ns, st))) return launch_failed(rc, F.what);
    HIPCHK(hipMemcpyAsync(d_carry, F.prim_carry.p, sizeof(float) * ns * kLevelCarry, hipMemcpyDeviceToDevice, st));
    return 0;
}

int levels_prim_host(LevelFollower& F, hipStream_t st, size_t ns, const std::function<int()>& thresholds, const float* power,
                     size_t frames, float* carry, uint8_t* levels) {
    const size_t n_pow = ns * frames * kMeterTones, n_lv = ns * level_row_bytes(F.K, frames);
    // the powers, then the carry, in one buffer of floats; the level rows in the follower's
    int rc = F.prim_pow.ensure(n_pow + ns * kLevelCarry);
    if (rc || (rc = F.levels.ensure(n_lv))) return rc;
    float* d_carry = F.prim_pow.p + n_pow;
    HIPCHK(hipMemcpyAsync(F.prim_pow.p, power, sizeof(float) * n_pow, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_carry, carry, sizeof(float) * ns * kLevelCarry, hipMemcpyHostToDevice, st));
    if ((rc = levels_prim_device(F, st, ns, thresholds, F.prim_pow.p, frames, d_carry, F.levels.p))) return rc;
    HIPCHK(hipMemcpyAsync(levels, F.levels.p, n_lv, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(carry, d_carry, sizeof(float) * ns * kLevelCarry, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace fmrx
