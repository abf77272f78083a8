// levels.h — the level follower: what the stages that follow the meter per frame share on the host (soft
// stereo, K = 1 level byte a frame; quieting, K = 2).  A stage's levels kernel turns the meter's powers
// into rows of level bytes 0 .. 16, entry 0 of a row the carried-in level(s); the follower owns those rows,
// the eight floats a stream the kernel carries from call to call, the "hold" form that repeats each
// stream's last level(s), and the copy back that the stage counts into its reports.  It needs no context:
// a stream, a stream count and the stage's launch function.  ctx.h includes this behind its buffer types
// (include ctx.h, not this); levels.cpp holds the code, tools/check_level_follower.cpp checks it on the CPU.
#pragma once

namespace fmrx {

constexpr int kLevelCarry = 8;      // floats a stream carried from call to call
constexpr unsigned kLevelMax = 16;  // a level byte counts as at most this
static_assert(kBlendCarry == kLevelCarry && kQuietCarry == kLevelCarry, "the stages' levels kernels carry eight floats a stream");
static_assert(kBlendSteps == (int)kLevelMax && kQuietSteps == (int)kLevelMax, "the stages' levels are 0 .. 16");

// bytes a stream's row of `frames` frames takes: the carried-in entry, then one a frame
inline size_t level_row_bytes(int K, size_t frames) { return (size_t)K * (frames + 1); }

struct LevelFollower {
    using Launch = int (*)(const LevelsLaunch&, int n_streams, hipStream_t);
    // one stream's frames of a call into the stage's reports: `frames` entries of K bytes, each 0 .. 16
    using CountRow = void (*)(void* reports, size_t stream, const uint8_t* row, size_t frames);
    LevelFollower(int k, Launch l, const char* w) : K(k), launch(l), what(w) {}
    const int K;                          // level bytes a frame
    const Launch launch;                  // the stage's levels kernel
    const char* const what;               // its name in a launch failure
    PingPong<float> carry;                // n_streams x kLevelCarry
    DevBuf<uint8_t> levels;               // a call's level rows: n_streams x K (frames + 1)
    std::vector<uint8_t> host;            // their host copy without entry 0 (K frames bytes a stream)
    size_t pending = 0;                   // frames a stream of a call enqueued and not yet counted
    bool hold = false;                    // calls run at the streams' last levels
    std::vector<uint8_t> last;            // n_streams x K: the level(s) of the last frame counted (0 after a reset)
    std::vector<uint8_t> hold_rows;       // a held call's level rows on the host
    DevBuf<float> prim_thr, prim_carry;   // the levels primitive's: a caller's thresholds (the stage fills them), the next carry before it is copied back
    DevBuf<float> prim_pow;               // its host form's: the caller's powers, then the carry
    // bytes between the rows of the call enqueued: the apply kernel's level_stride
    size_t stride() const { return level_row_bytes(K, pending); }
};

// the carry (once it exists) zeroed and rewound, `last` cleared, nothing pending, hold off
int levels_reset(LevelFollower& F, hipStream_t st, size_t ns);
// a call's frames: the levels kernel over the meter's powers with the stage's thresholds, enqueued, the carry moved
int levels_enqueue(LevelFollower& F, hipStream_t st, size_t ns, const float* d_power, const float* d_thr, size_t frames);
// a call under hold: every entry of a stream's row its last level(s), `held` frames and the carried-in one;
// the rows go up by a blocking copy
int levels_enqueue_held(LevelFollower& F, hipStream_t st, size_t ns, size_t held);
// the level bytes of the call enqueued copied back (without entry 0) and clamped, the stream waited for, one
// `count` a stream, the last frame's bytes kept; under hold nothing was measured and nothing is counted
int levels_finish(LevelFollower& F, hipStream_t st, size_t ns, LevelFollower::CountRow count, void* reports);
// the frames a levels primitive takes: 1 .. (2^31 - 1) / 7 (FMRX_EINVAL otherwise)
int levels_check_frames(size_t frames);
// the levels primitive: the kernel over d_power with a caller's carry (in and out) and rows; `thresholds`
// has the stage put the caller's config's thresholds into prim_thr (or refuse the config)
int levels_prim_device(LevelFollower& F, hipStream_t st, size_t ns, const std::function<int()>& thresholds, const float* d_power,
                       size_t frames, float* d_carry, uint8_t* d_levels);
// its host form (frames checked by the caller, before the device is set): powers and carry up, rows and carry back
int levels_prim_host(LevelFollower& F, hipStream_t st, size_t ns, const std::function<int()>& thresholds, const float* power,
                     size_t frames, float* carry, uint8_t* levels);

}  // namespace fmrx
