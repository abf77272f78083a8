// ctx.h — what the host runtime's files share: the context, its buffers, the error text and the
// functions that cross files.  Private to the host sources (context.cpp, engine.cpp, front.cpp,
// process.cpp, rds_api.cpp, rds_sync_api.cpp, meter_api.cpp, levels.cpp, blend_api.cpp, quiet_api.cpp, afc_api.cpp, scan_api.cpp, prims_api.cpp); no .hip file includes it.  No CPU compute path exists:
// every numeric result comes from a GPU kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fmrx.h"
#include "fmrx_internal.h"
#include "tuner.h"
#include "wide.h"

namespace fmrx {

// sets the calling thread's fmrx_last_error() text and returns code (context.cpp)
int fail(int code, const char* fmt, ...);

#define HIPCHK(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(FMRX_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                        __FILE__, __LINE__);                                           \
    } while (0)

constexpr int kDemodHist = 64;   // demod samples kept in front of each call (>= bp_taps-1)
constexpr int kMixTail = 64;     // must match stereo.hip kTail
constexpr int kAudioHist50 = 50;  // demod samples a resampler output reads before its base
// calls up to this many input bytes go through the pinned staging (larger ones: device buffers
// and hipMemcpyAsync, whose DMA beats kernels reading host memory at that size)
constexpr size_t kPinnedCallBytes = (size_t)4 << 20;

// Memory of `count` T that its holder owns, on the device or (kPinned) pinned on the host: grown by
// ensure() (the old contents are dropped), given back by release() or by the destructor.  Never copied;
// moved only where a grown buffer replaces the one it preserves (engine.cpp grow_rows).  A context's
// buffers are freed by `delete` in fmrx_destroy, once the device is set and every stream is drained.
template <class T, bool kPinned>
struct Buf {
    T* p = nullptr;
    size_t n = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(Buf&& o) noexcept {  // (so no copy assignment either) o leaves with this one's old memory
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~Buf() { release(); }
    int ensure(size_t count) {
        if (count <= n) return 0;
        release();
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        void* q = nullptr;
        if ((kPinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes)) != hipSuccess)
            return fail(FMRX_ENOMEM, "%s of %zu bytes failed", kPinned ? "hipHostMalloc" : "hipMalloc", count * sizeof(T));
        p = static_cast<T*>(q);
        n = count;
        return 0;
    }
    void release() {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        n = 0;
    }
};
template <class T>
using DevBuf = Buf<T, false>;
// Pinned host memory, mapped into the device's address space (hipHostMalloc: kernels read and
// write it through the same pointer): the staging of the host-buffer entry points' small calls
// (the reference's per-block seam, project.cpp:48-84 / 132-196): the input goes to the device by
// DMA from it, the kernels write their output into it in place -- one copy operation on the stream
// and one host memcpy each way.
template <class T>
using PinnedBuf = Buf<T, true>;
static_assert(!std::is_copy_constructible_v<DevBuf<float>> && !std::is_copy_assignable_v<DevBuf<float>>);
static_assert(!std::is_copy_constructible_v<PinnedBuf<float>> && !std::is_copy_assignable_v<PinnedBuf<float>>);

// Two device buffers and a cursor: a launch reads cur() and writes next(), the host flips once the
// launch is enqueued; a reset rewinds to the first buffer.
template <class T>
struct PingPong {
    DevBuf<T> buf[2];
    int at = 0;
    T* cur() const { return buf[at].p; }
    T* next() const { return buf[at ^ 1].p; }
    void flip() { at ^= 1; }
    void rewind() { at = 0; }
    int ensure(size_t count) {
        const int rc = buf[0].ensure(count);
        return rc ? rc : buf[1].ensure(count);
    }
};

// src into d, grown to count, by a blocking copy (creation's tables; `what` words the failure)
template <class T>
int upload(DevBuf<T>& d, const T* src, size_t count, const char* what) {
    const int rc = d.ensure(count);
    if (rc) return rc;
    return hipMemcpy(d.p, src, sizeof(T) * count, hipMemcpyHostToDevice) == hipSuccess ? 0 : fail(FMRX_EHIP, "%s failed", what);
}

// a launch function's code as the entry point's: "<what> launch failed (rc)", FMRX_EINVAL for -1 (then with `hint`)
inline int launch_failed(int rc, const char* what, const char* hint = "") {
    return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "%s launch failed (%d)%s", what, rc, rc == -1 ? hint : "");
}

}  // namespace fmrx

#include "levels.h"  // the level follower (it needs the buffer types above)

namespace fmrx {

using TimingPair = std::pair<hipEvent_t, hipEvent_t>;

// The rate of a context's captures against the mode's: cap_fs = rf_fs down / up in lowest terms.  1/1:
// no wide stage; up = 1: the integer stage (wide.hip); anything else: the rational one (rate.hip).
// Everything the host derives from the ratio has one form; the integer case is that form at up = 1.
struct CaptureRatio {
    int up = 1, down = 1;
    size_t blocks = 1;  // narrow blocks a granule (the fewest that are whole wide pairs): up / gcd(up, iq_pairs)
    bool on() const { return down != up; }
    bool rational() const { return up != 1; }
    int cap_fs(int rf_fs) const { return rf_fs / up * down; }  // up divides rf_fs
    // raw wide pairs of history the stage keeps in front of the next call
    size_t hist_pairs() const { return (size_t)rate_hist_pairs(up, down); }
    // wide pairs that n_blocks narrow blocks of iq_pairs take (n_blocks a whole number of granules)
    size_t pairs_of(size_t n_blocks, size_t iq_pairs) const { return n_blocks * iq_pairs / (size_t)up * (size_t)down; }
    // wide pairs a narrow pair, rounded up: check_call_size's factor of a wide call
    size_t size_factor() const { return (size_t)((down + up - 1) / up); }
};

// bounds on the streams' trigOffset (PllHint) of the stereo and the RDS PLL: 0 after a reset,
// advanced by every call's samples (the float increments stick at 2^24), re-read from the
// blob by fmrx_set_state; unknown after a failed launch
struct TrigTrack {
    bool known = true;
    double lo = 0.0, hi = 0.0;
    void advance(size_t n) {
        lo = std::min(lo + (double)n, 16777216.0);
        hi = std::min(hi + (double)n, 16777216.0);
    }
};

// The members of fmrx_ctx (below: the ABI's opaque type lives outside the namespace).
struct Ctx {
    mutable std::recursive_mutex mu;  // every entry point holds it: one call on a context at a time
    fmrx_config cfg{};
    fmrx_geometry_t geo{};
    hipStream_t stream = nullptr;
    int n_simd = 1024;                        // SIMDs of cfg.device (4 per CU), set at creation
    // One struct a stage: the buffers, strides, switches, host copies and pending counters it owns.  A
    // buffer added to one of them needs no edit outside that struct and the stage's own code.
    // The first: the filter taps on the host and their device copies, designed and uploaded at creation.
    struct Taps {
        std::vector<float> rf, audio, ch, ca;
        MonoTaps mono{};
        DevBuf<float> d_audio, d_rf;
        DevBuf<float> d_audio_rows;   // modes 2/3: the audio prototype by phase (kAudioRow floats per row)
    } taps;
    // The raw-I/Q front: the raw bytes preceding the next call, double-buffered (in the checkpoint blob;
    // allocated at creation, regrown by fmrx_set_input_format).
    struct Front {
        size_t halo_bytes = 0;        // halo_pairs * pair_bytes
        size_t halo_pairs = 0;
        int format = kIqU8;           // fmrx_set_input_format: the raw I/Q format of every stream
        size_t pair_bytes = 2;        // bytes an I/Q pair of it
        PingPong<uint8_t> halo;
    } front;
    // Audio state of the mono product: the last hist_len (audio_taps_total - 1) demod samples a stream (in the
    // blob; allocated at creation).
    struct MonoAudio {
        int hist_len = 0;
        DevBuf<float> hist;
        bool stale = false;           // after fmrx_seek, until a fused call refreshes it
    } mono;
    // The stereo engine.  Demod history, PLL state, mix tail and mono state are in the blob and allocated at
    // creation; the rows grow with the calls; the pipelined engine (run_stereo_pipelined) creates its
    // front-end / band-pass stream, audio stream and events at the first pipelined call.
    struct Stereo {
        DevBuf<float> demod;          // n_streams x (kDemodHist + cap_if)
        size_t demod_stride = 0;
        DevBuf<float> channel, carrier;
        DevBuf<float> pll;            // n_streams x 8
        DevBuf<float> mix_tail;       // n_streams x kMixTail
        DevBuf<float> mono_state;     // n_streams x 8
        DevBuf<double> pll_side;      // PLL side data of one segment (pll_side_doubles)
        DevBuf<double> pll_side2;     // the pipelined engine's second one (odd chunks: their NCO runs
                                      //   on the audio stream while the next chunk's PLL fills the first)
        TrigTrack trig;
        hipStream_t s_front = nullptr, s_audio = nullptr;  // destroyed by fmrx_destroy, with the context stream
        std::vector<hipEvent_t> pipe_ev;
        ~Stereo() {
            for (auto e : pipe_ev) (void)hipEventDestroy(e);
        }
    } stereo;
    // RDS front half (project.cpp:200-271; not part of the checkpoint blob): taps, history and PLL state at
    // creation, the rows grown with the calls.
    struct RdsFront {
        DevBuf<float> taps;           // 54-60 kHz taps, then 113.5-114.5 kHz taps
        DevBuf<float> dhist;          // n_streams x kRdsDemodHist
        DevBuf<float> chan;           // n_streams x (kRdsChanHist + cap)
        size_t chan_stride = 0;
        DevBuf<float> car;            // n_streams x cap
        DevBuf<float> pll;            // n_streams x 8
        TrigTrack trig;
    } rds;
    // RDS back half (rds_bits.hip; not part of the checkpoint blob either): taps, history and state at
    // creation, the rest grown with the calls.
    struct RdsBits {
        DevBuf<float> taps;           // kRdsbTaps: impulseResponseLPF(19 bp_fs, 3000, 1919, 19)
        DevBuf<float> hist;           // n_streams x kRdsbHist mixer samples in front of the next call
        DevBuf<uint8_t> state;        // n_streams x kRdsbStateBytes
        DevBuf<uint8_t> work;         // a call's signs, phases, last chips and symbols
        DevBuf<float> mix;            // fmrx_rds_decode*: the front half's mixer rows
        DevBuf<uint8_t> out;          // fmrx_rds_decode*: bits, then codes
        std::vector<uint8_t> host;    // their host copy, read by the parser
        size_t pending = 0;           // symbols a stream of a decode enqueued and not yet parsed
        std::vector<fmrx_rds_info> info;  // n_streams
        bool on = false;              // fmrx_set_rds
    } rdsb;
    // RDS block sync (fmrx_set_rds_sync, rds_sync.hip; not part of the checkpoint blob): nothing here is
    // allocated until the switch is first turned on (or fmrx_rds_blocks first runs)
    struct RdsSync {
        bool on = false;                      // fmrx_set_rds_sync
        fmrx_rds_sync_config cfg{8, 3, 2};    // the constants the streams began with
        int table_b = -1;                     // the B `table` holds (-1: none yet)
        uint64_t seen = 0;                    // bits a stream has been given since the reset
        uint64_t judged = 0;                  // positions below it are judged
        DevBuf<uint32_t> table;               // kRdsSyncTable burst patterns
        DevBuf<uint8_t> carry;                // n_streams x kRdsSyncCarry: the last bits, right-aligned
        DevBuf<uint32_t> work;                // a call's candidates, records and exact masks
        DevBuf<uint8_t> in;                   // fmrx_rds_blocks: the caller's bit rows
        DevBuf<fmrx_rds_block_rec> blocks;    // the host forms' lists: n_streams x the positions judged
        DevBuf<uint32_t> counts;              // n_streams
        std::vector<uint32_t> counts_host;    // their host copies: the counts, and `most` records a stream
        std::vector<fmrx_rds_block_rec> host;
        size_t most = 0;
        bool pending = false;                 // a decode enqueued the stage and has not yet parsed its records
        size_t cap = 0, bits = 0;             //   its list rows and its bits a stream
        std::vector<fmrx_rds_ext> ext;        // n_streams
    } rdss;
    // the frame geometry of the mode (set at creation): a granule without a capture rate is the fewest
    // blocks that are whole meter frames
    struct Frames {
        unsigned A = 0, Gm = 0;               // audio frames and meter frames a granule
    } frames;
    // subcarrier meter (fmrx_set_meter, meter.hip): no signal state; nothing here is allocated until the
    // switch is first turned on (or fmrx_meter first runs)
    struct Meter {
        bool on = false;                      // fmrx_set_meter
        int p = 0;                            // samples a window (bp_fs / 1000) once `tab` is filled
        DevBuf<float> tab;                    // the 14 tables of fmrx_meter_design
        DevBuf<float> pow;                    // a call's powers: n_streams x frames x 7
        std::vector<float> host;              // their host copy
        size_t pending = 0;                   // frames a stream of a call enqueued and not yet added
        std::vector<fmrx_meter_report> rep;   // n_streams
    } meter;
    // AFC (fmrx_set_afc, afc.hip): the carrier sums of the demod rows, the decisions and the retunes; no
    // signal state, not in the blob; nothing on the device is allocated until the switch is first turned on
    // (or fmrx_carrier first runs).  The offsets it moves are tune.offsets, or wide.offsets once
    // fmrx_tune_wide was accepted (`wide` says which the origins are)
    struct Afc {
        bool on = false;                      // fmrx_set_afc
        fmrx_afc_config cfg{1000, 1000, 50000, 16, 1, 1.0f};
        DevBuf<float> sums;                   // a call's sums: n_streams x frames x 2
        std::vector<float> host;              // their host copy
        size_t pending = 0;                   // frames a stream of a call enqueued and not yet added
        std::vector<fmrx_carrier_report> total, window;  // n_streams: since the reset, since the last decision
        std::vector<int32_t> origin;          // n_streams: what the caller last tuned to
        bool wide = false;                    // the origins are fmrx_tune_wide's
        bool moved = false;                   // some offset is not its origin
        std::vector<uint32_t> retunes, refused, decisions;  // n_streams
        std::vector<fmrx_afc_decision> last;  // n_streams
    } afc;
    // FM de-emphasis (fmrx_set_deemphasis, deemph.hip): configuration and a carry of its own, not in the
    // blob; nothing here is allocated until it is first turned on (or fmrx_deemph first runs)
    struct Deemph {
        int tau = 0;                          // 0 off, 50 or 75 us
        DevBuf<float> taps;                   // 2 x kDeemphTaps: the context's audio rate at 50, then at 75 us
        PingPong<float> state;                // n_streams x channels x kDeemphHist inputs in front of the next call
        DevBuf<float> x;                      // a call's floats in front of the quantiser (4 B a sample and channel)
        DevBuf<float> tmp;                    // fmrx_deemph: the caller's next state, before it is copied back
    } deemph;
    // soft stereo (fmrx_set_stereo_blend, blend.hip): configuration and a level follower of its own (levels.h),
    // not in the blob; nothing here is allocated until the switch is first turned on (or a blend primitive
    // first runs)
    struct Blend {
        bool on = false;                      // fmrx_set_stereo_blend
        fmrx_blend_config cfg{10.0f, 22.0f};
        float c = 0.0f;                       // (float)(1.0 / (32.0 frames.A))
        DevBuf<float> thr;                    // the 16 thresholds of cfg
        LevelFollower f{1, launch_blend_levels, "blend levels"};  // fmrx_blend_hold sets its hold
        std::vector<fmrx_blend_report> rep;   // n_streams
        fmrx_blend_config prim_cfg{0.0f, 0.0f};  // the config f.prim_thr holds (lo == hi: none yet)
    } blend;
    // quieting (fmrx_set_quieting, quiet.hip): configuration, a level follower (levels.h) and a history of its
    // own, not in the blob; nothing here is allocated until the switch is first turned on (or a quieting
    // primitive first runs)
    struct Quiet {
        bool on = false;                      // fmrx_set_quieting
        fmrx_quiet_config cfg{22.0f, 34.0f, 36.0f, 44.0f, 20.0f, 2500};
        float g0 = 0.0f, cg = 0.0f, cw = 0.0f;  // cfg's gains once `tab` is filled
        DevBuf<float> tab;                    // cfg's Tc (16), Tm (16) and taps (64)
        LevelFollower f{2, launch_quiet_levels, "quieting levels"};  // a frame's pair (c, m); fmrx_quiet_hold sets its hold
        PingPong<float> hist;                 // n_streams x channels x kQuietHist inputs in front of the next call
        DevBuf<float> x;                      // a call's output floats when de-emphasis follows
        std::vector<fmrx_quiet_report> rep;   // n_streams
        fmrx_quiet_config prim_cfg{};         // the config f.prim_thr holds (all zero: none yet)
        DevBuf<float> prim_hist;              // fmrx_quiet_apply_device: the caller's next history, before it is copied back
    } quiet;
    // off-centre tuning (fmrx_tune): configuration, not part of the state blob; the tables are allocated
    // by the first fmrx_tune or by a format other than u8
    struct Tuner {
        bool on = false;
        std::vector<int32_t> offsets;         // n_streams (zeros until fmrx_tune sets them)
        uint64_t pos = 0;                     // absolute pair index of the next call's first I/Q pair
        int max_n = 1;                        // the longest rotator period among the streams
        DevBuf<float> tab;                    // the streams' (c, s) tables, one after the other
        DevBuf<uint32_t> streams;             // TunerStream per stream
    } tune;
    // wide captures (fmrx_set_capture_decim, fmrx_set_capture_rate): the capture stage in front of the
    // tuner (wide.hip or rate.hip, by the ratio); its history, rows and narrow halo are its own, nothing
    // the ordinary calls read or the blob holds; allocated when a ratio other than 1/1 is set
    struct Wide {
        CaptureRatio ratio;                   // cap_fs / rf_fs; 1/1: no wide stage
        bool tuned = false;                   // fmrx_tune_wide accepted (fmrx_tune turns it off)
        std::vector<int32_t> offsets;         // n_streams, against cap_fs
        DevBuf<uint8_t> hist;                 // the ratio.hist_pairs() raw pairs of the capture in front of the next call
        DevBuf<float> taps;                   // the low-pass: 16 down + 1 floats at up = 1, else the RateTap rows by phase
        DevBuf<float> tab;                    // n_streams x kRateMaxN (c, s) pairs: the coarse tables
        DevBuf<uint32_t> streams;             // WideStream per stream
        DevBuf<float> y;                      // n_streams x y_stride floats: one piece's cf32 rows at rf_fs
        size_t y_stride = 0;
        PingPong<uint8_t> halo;               // the narrow stage's f32 halo (halo_pairs x 8 B a stream)
    } wide;
    // band scan (fmrx_scan*): scratch of its own, grown on demand; nothing the decode path reads
    struct Scan {
        int bins = 0;                         // the transform size `tab` holds (0: none yet)
        std::vector<float> tab_host;          // host copy: 2 N twiddle floats, then N window floats
        DevBuf<float> tab;                    // the same on the device
        DevBuf<float> part;                   // the launch's partial rows (scan_workgroups x N)
        DevBuf<float> power;                  // the host entry points' result, N floats
        DevBuf<uint8_t> in;                   // the host entry points' capture
    } scan;
    // staging for the host-buffer entry points and the primitives' scratch, grown with the calls
    struct Staging {
        DevBuf<uint8_t> d_in;
        DevBuf<int16_t> d_out;
        PinnedBuf<uint8_t> h_in, h_out;       // the small host calls' staging (kPinnedCallBytes)
        DevBuf<float> f32;
        DevBuf<float> scratch;
    } io;
    // the synthetic input: the sine table (creation) and fmrx_synth_device_streams' SynthParams per stream
    struct Synth {
        DevBuf<int16_t> sintab;
        DevBuf<uint8_t> params;
    } synth;
    // diagnostics.  Kernel timing: pairs of HIP events recorded around each fused-kernel launch on the
    // context stream (no host sync inside the timed loop); read by fmrx_kernel_timing.  The three raw
    // pointers are device memory of the caller's: never owned, never freed here.
    struct Diag {
        std::vector<TimingPair> evs;
        size_t ev_used = 0;
        bool timing = false;
        unsigned long long* stamps = nullptr;     // fmrx_debug_mono_stamps (caller-owned)
        unsigned long long* pll_stats = nullptr;  // fmrx_debug_pll_stats (caller-owned)
        unsigned* pll_redos = nullptr;            // fmrx_debug_pll_redos (caller-owned)
        StageTimer timer;                         // fmrx_debug_stage_timing
        ~Diag() {
            for (auto& e : evs) (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
            timer.release();
        }
    } diag;
    // switches (fmrx_debug_set_knob): the tuning ones from the environment once, at creation;
    // none of them changes the output (the PLL test hooks make the runners redo work)
    struct Knobs {
        PllKnobs pll;
        int stereo_chunks = 0;  // 0: by stream count and call length; k: k chunks (1: serial engine)
        int stereo_head = 8;    // the first chunk's blocks in 16ths of a middle chunk's
        int stereo_tail = 8;    // the last chunk's blocks in 16ths of a middle chunk's
        int stereo_lead = 0;    // n > 0: chunk k's front end waits for chunk k - n's PLL; 0: none
        int audio_defer = 2;    // 2: chunks 0 .. K-2's audio beside the last PLL; 1: all after it; 0: beside the next
                                // (2 + e: chunks 0 .. e-1 beside the PLL before the last)
        int mono_split = -1;    // -1: kOlderShare; 0: equal spans; n: the older wave's n / 1024
        int bpf_tile = 1;       // 0: the per-output band-pass kernel
        int halo_kernel = 0;    // 1: the separate halo_kernel after the fused one
    } knobs;
    PllHint hint(const TrigTrack& t) const {
        PllHint h;
        h.n_simd = n_simd;
        h.knobs = knobs.pll;
        h.redos = diag.pll_redos;
        h.known = t.known;
        h.trig_lo = t.lo;
        h.trig_hi = t.hi;
        h.timer = diag.timer.on ? const_cast<StageTimer*>(&diag.timer) : nullptr;
        return h;
    }
};

}  // namespace fmrx

struct fmrx_ctx : fmrx::Ctx {};

namespace fmrx {

// Serialises the entry points of one context (rf and audio stages may be driven from two
// threads, as project.cpp does; they share the context's stream and scratch buffers).
class CtxLock {
  public:
    explicit CtxLock(const fmrx_ctx* c) : c_(c) {
        if (c_) c_->mu.lock();
    }
    ~CtxLock() {
        if (c_) c_->mu.unlock();
    }
    CtxLock(const CtxLock&) = delete;
    CtxLock& operator=(const CtxLock&) = delete;

  private:
    const fmrx_ctx* c_;
};

// The byte that fills a run of x = 0.0 samples of the context's format
inline int iq_zero_byte(const fmrx_ctx* c) { return c->front.format == kIqU8 ? 0x80 : 0; }
// Bytes a block of one stream's raw I/Q takes in the context's format (geo.block_bytes for u8)
inline size_t iq_block_bytes(const fmrx_ctx* c) { return c->geo.iq_pairs * c->front.pair_bytes; }
// The calls that take raw I/Q run the tuned front end (tuner.hip) while tuning is on, and always
// for a format other than u8 (the fused kernels read u8 only): with tuning off the context's
// tables then hold zero offsets, which gives the untuned bits.
inline bool front_tuned(const fmrx_ctx* c) { return c->tune.on || c->front.format != kIqU8; }
// n_streams rows of n_blocks blocks in format bytes must fit size_t with room to spare (a block of
// f32 is four times a block of u8)
inline int check_call_size(const fmrx_ctx* c, size_t n_blocks, size_t decim = 1) {
    const size_t per_block = (size_t)c->cfg.n_streams * c->geo.iq_pairs * 8 * decim;  // decim: a wide block
    if (n_blocks > (std::numeric_limits<size_t>::max() / 4) / per_block)
        return fail(FMRX_EINVAL, "%zu blocks: the call's byte count overflows", n_blocks);
    return 0;
}
// Wide pairs that n_blocks narrow blocks take (n_blocks a whole number of granules)
inline size_t wide_pairs_of(const fmrx_ctx* c, size_t n_blocks) { return c->wide.ratio.pairs_of(n_blocks, c->geo.iq_pairs); }
inline int set_device(const fmrx_ctx* c) {
    HIPCHK(hipSetDevice(c->cfg.device));
    return 0;
}
// `count` floats at src into d, grown to hold them; the stream is drained first (a launch in flight may
// still read the old ones)
inline int upload_floats(fmrx_ctx* c, const float* src, size_t count, DevBuf<float>& d) {
    const int rc = d.ensure(count);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(d.p, src, sizeof(float) * count, hipMemcpyHostToDevice));
    return 0;
}
// meter frames of n_blocks blocks (whole granules): the frames of the meter, the carrier sums and the levels
inline size_t meter_frames(const fmrx_ctx* c, size_t n_blocks) {
    return n_blocks * c->geo.if_samples / ((size_t)kMeterWindows * (size_t)(c->geo.bp_fs / 1000));
}

// Every stage that keeps signal state has an init_ (creation: its tables designed and uploaded, its
// creation-time buffers allocated) and a reset_ (its start state, enqueued on the context stream) beside
// its code; fmrx_create and reset_state (context.cpp) call them in turn.  pll0: the PLL start vector.

// ---- context.cpp
int reset_state(fmrx_ctx* c);
// fmrx_kernel_timing around one launch on st: when timing is armed, begin takes the next event pair
// and records its first event (*ev, null at the call, stays null otherwise); end records the second
int timing_begin(fmrx_ctx* c, hipStream_t st, TimingPair** ev);
inline int timing_end(TimingPair* ev, hipStream_t st) {
    if (ev) HIPCHK(hipEventRecord(ev->second, st));
    return 0;
}

// ---- engine.cpp
int init_audio(fmrx_ctx* c);   // the RF and audio taps, the mono history, the stereo state
int reset_audio(fmrx_ctx* c, const std::vector<float>& pll0);
int init_rds_front(fmrx_ctx* c);
int reset_rds_front(fmrx_ctx* c, const std::vector<float>& pll0);
int reset_deemph(fmrx_ctx* c);  // the de-emphasis carry alone (nothing to do before it was ever on)
// RF front end (+ the mono audio stage when `with_audio`); the chunk form serves the stereo pipeline
int run_fused(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm, float* d_mono, float* d_demod,
              size_t demod_stride, int demod_hist, bool with_audio, size_t b0 = 0, size_t call_blocks = 0,
              hipStream_t st = nullptr, bool last = true);
int run_mono_audio(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_if, int16_t* d_pcm, float* d_mono);
int run_stereo_audio(fmrx_ctx* c, size_t n_blocks, int16_t* d_pcm, float* d_mono, const float* src = nullptr);
int stereo_chunks(const fmrx_ctx* c, size_t n_blocks);
int run_stereo_pipelined(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm, float* d_mono, int K);
int run_rds(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_if, float* d_out, float* d_nco,
            float* d_channel);
int ensure_demod(fmrx_ctx* c, size_t n_if);
// De-emphasis behind an audio stage (fmrx_set_deemphasis on): the taps, and the audio rate they are designed for
int ensure_deemph_taps(fmrx_ctx* c);
inline int deemph_audio_fs(const fmrx_ctx* c) { return c->geo.if_fs / c->geo.audio_down; }  // if_fs holds audio_up

// ---- rds_api.cpp
// blocks of an RDS granule (with a capture rate set: the least common multiple with the wide granule's)
size_t rds_granule_blocks(const fmrx_ctx* c);
int check_rds_blocks(const fmrx_ctx* c, size_t n_blocks);
int init_rds_bits(fmrx_ctx* c);
int reset_rds_bits(fmrx_ctx* c);  // the back half's start state (and the block sync's)
// front half, bits and codes of the rows at d_demod (whole granules), and their copy to the host, enqueued;
// rds_decode_finish waits for the stream and parses them into rdsb.info
int rds_decode_enqueue(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_blocks);
int rds_decode_finish(fmrx_ctx* c);

// ---- rds_sync_api.cpp
void reset_rds_sync(fmrx_ctx* c);  // the carry's counters and the extended infos back to the start
// the block sync over n_bits more bits a stream at d_bits (rows n_bits apart) and the copy of its counts, enqueued;
// rds_sync_finish waits for the stream, fetches the records and parses them into rdss.ext
int rds_sync_enqueue(fmrx_ctx* c, const uint8_t* d_bits, size_t n_bits);
int rds_sync_finish(fmrx_ctx* c);

// ---- meter_api.cpp
void init_frames(fmrx_ctx* c);                               // the mode's frames.A and frames.Gm; nothing allocated
// whole frames: the RDS granule's blocks, or FMRX_EINVAL "<who> takes whole frames, granules of ..."
int check_frame_blocks(const fmrx_ctx* c, size_t n_blocks, const char* who);
void reset_meter(fmrx_ctx* c);                               // the reports back to zero
// the meter's tables on the device by fmrx_set_meter's own path, its switch put back as it was (the stages
// that read its powers call this when they are turned on)
int meter_tables_ready(fmrx_ctx* c);
// the meter over the rows at d_demod (whole frames) and the copy of its powers to the host, enqueued;
// meter_finish waits for the stream and adds them to the streams' reports
int meter_enqueue(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_blocks);
int meter_finish(fmrx_ctx* c);

// ---- afc_api.cpp
void reset_afc_reports(fmrx_ctx* c);                         // reports, decisions and counts back to zero (sized here)
int reset_afc(fmrx_ctx* c);                                  // that, and the offsets back to the origins
void afc_caller_tuned(fmrx_ctx* c);                          // fmrx_tune / fmrx_tune_wide accepted: new origins, windows cleared
// the carrier sums over the rows at d_demod (whole frames), enqueued; afc_finish copies them back, waits for
// the stream, adds them to the reports and, with tracking on, decides and retunes
int afc_enqueue(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_blocks);
int afc_finish(fmrx_ctx* c);

// ---- blend_api.cpp, quiet_api.cpp: the two stages on a level follower.  A tuned call enqueues the follower
// over the powers the meter kernel left in meter.pow (front.cpp taps_enqueue: levels_enqueue, or
// levels_enqueue_held under hold), runs the stage's apply kernel by the rows (engine.cpp quant_rows), and
// has the stage's finish count the level bytes into its reports
void init_blend(fmrx_ctx* c);                                // soft stereo's c of frames.A; nothing allocated
int reset_blend(fmrx_ctx* c);                                // the follower and the reports back to the start
int reset_quiet(fmrx_ctx* c);                                // that, and the history (once it exists)
inline bool blend_metered(const fmrx_ctx* c) { return c->blend.on && !c->blend.f.hold; }  // the call's levels come from the meter
inline bool quiet_metered(const fmrx_ctx* c) { return c->quiet.on && !c->quiet.f.hold; }
// the call's (right, left) rows through the apply kernel (out and pcm as BlendApplyLaunch's)
int blend_apply(fmrx_ctx* c, float* rows, size_t na, bool in_place, int16_t* d_pcm);
// the call's rows (na frames a stream) through the apply kernel into d_out (floats), d_pcm or both, the history moved
int quiet_apply(fmrx_ctx* c, const float* rows, size_t na, float* d_out, int16_t* d_pcm);
int blend_finish(fmrx_ctx* c);
int quiet_finish(fmrx_ctx* c);
// "<who>: not with soft stereo on (<why>)", then "... quieting on (<why_quiet>, or <why>)", as FMRX_ESTATE
// while that switch is on, else 0
inline int refuse_row_stages(const fmrx_ctx* c, const char* who, const char* why, const char* why_quiet = nullptr) {
    if (c->blend.on) return fail(FMRX_ESTATE, "%s: not with soft stereo on (%s)", who, why);
    return c->quiet.on ? fail(FMRX_ESTATE, "%s: not with quieting on (%s)", who, why_quiet ? why_quiet : why) : 0;
}

// ---- front.cpp
int init_front(fmrx_ctx* c);   // the halo; the tuner's and the wide stage's per-stream offsets
int reset_front(fmrx_ctx* c);  // the halo and the position; the offsets stay (configuration)
int reset_wide(fmrx_ctx* c);   // nothing to do at 1/1
int run_tuned_front(fmrx_ctx* c, const uint8_t* d_iq, size_t iq_stride, size_t n_blocks, float* d_demod,
                    size_t demod_stride, int demod_hist, bool pre_tail);
int run_tuned(fmrx_ctx* c, const uint8_t* d_iq, size_t iq_stride, size_t n_blocks, int16_t* d_pcm, float* d_mono);
int run_wide(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm);
// decim within the down-converter's range (or_one: 1, no wide stage, passes too); rf_fs a positive multiple of 4
int check_capture_decim(int decim, bool or_one);
int check_wide_rf_fs(int rf_fs);
// n_blocks of a wide call: whole granules (FMRX_EINVAL otherwise)
int check_wide_blocks(const fmrx_ctx* c, size_t n_blocks);
// what fmrx_tune (offsets non-null) and fmrx_tune_wide do once their arguments are checked; AFC's retunes run them too
int tune_narrow(fmrx_ctx* c, const int32_t* offsets_hz, uint64_t first_pair);
int tune_wide(fmrx_ctx* c, const int32_t* offsets_hz, uint64_t first_pair);

}  // namespace fmrx
