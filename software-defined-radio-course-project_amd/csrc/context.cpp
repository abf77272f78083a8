// context.cpp — the context of the C ABI (include/fmrx.h): error text, configuration and geometry,
// knobs, creation and destruction, reset and seek, the state blob, synchronisation and the timing
// read-outs.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctx.h"

using namespace fmrx;

namespace {

thread_local std::string g_err;

constexpr uint32_t kStateMagic = 0x46524D58u;  // "FMRX"
constexpr uint32_t kStateVersion = 2;  // 2: + flags word (bit 0: audio history stale after fmrx_seek)
constexpr int kStateHdrWords = 10;  // magic, version, mode, channels, rf_taps, n_streams, halo, audio_hist, flags, 0

bool fused_rf_supported(const fmrx_ctx* c) {
    const int t = c->geo.rf_taps, d = c->geo.rf_decim;
    return (t == 51 || t == 101) && (d == 10 || d == 4 || d == 9);
}

}  // namespace

namespace fmrx {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int timing_begin(fmrx_ctx* c, hipStream_t st, TimingPair** ev) {
    if (!c->diag.timing) return 0;
    if (c->diag.ev_used == c->diag.evs.size()) {
        TimingPair e{nullptr, nullptr};
        HIPCHK(hipEventCreate(&e.first));
        HIPCHK(hipEventCreate(&e.second));
        c->diag.evs.push_back(e);
    }
    *ev = &c->diag.evs[c->diag.ev_used++];
    HIPCHK(hipEventRecord((*ev)->first, st));
    return 0;
}

int reset_state(fmrx_ctx* c) {
    // project.cpp:106-111: integrator 0, phaseEst 0, feedbackI 1, feedbackQ 0, ncoOut_state 1,
    // trigOffset 0; RDS (project.cpp:206-226) starts its PLL the same
    std::vector<float> pll0(8 * (size_t)c->cfg.n_streams, 0.0f);
    for (size_t s = 0; s < pll0.size(); s += 8) pll0[s + 2] = pll0[s + 4] = 1.0f;
    int rc;
    if ((rc = reset_front(c)) || (rc = reset_wide(c)) || (rc = reset_audio(c, pll0)) || (rc = reset_rds_front(c, pll0)) ||
        (rc = reset_rds_bits(c)) || (rc = reset_deemph(c)) || (rc = reset_blend(c)) || (rc = reset_quiet(c)))
        return rc;
    reset_meter(c);
    if ((rc = reset_afc(c))) return rc;  // behind reset_front: a pulled stream goes back to its origin at position 0
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace fmrx

extern "C" {

const char* fmrx_last_error(void) { return g_err.c_str(); }
const char* fmrx_version(void) { return "fmrx 0.1 (gfx950)"; }

int fmrx_config_default(fmrx_config* cfg, int mode, int channels) {
    if (!cfg) return fail(FMRX_EINVAL, "null config");
    ModeConstants m;
    if (!mode_constants(mode, &m)) return fail(FMRX_EINVAL, "invalid mode %d", mode);
    if (channels != FMRX_MONO && channels != FMRX_STEREO)
        return fail(FMRX_EINVAL, "invalid channels %d", channels);
    cfg->mode = mode;
    cfg->channels = channels;
    cfg->rf_taps = 51;     // src/project.cpp:306
    cfg->bp_taps = 51;     // src/project.cpp:307
    cfg->audio_taps = 51;  // src/project.cpp:319
    cfg->n_streams = 1;
    cfg->device = 0;
    return FMRX_OK;
}

int fmrx_geometry(const fmrx_config* cfg, fmrx_geometry_t* g) {
    if (!cfg || !g) return fail(FMRX_EINVAL, "null argument");
    ModeConstants m;
    if (!mode_constants(cfg->mode, &m)) return fail(FMRX_EINVAL, "invalid mode %d", cfg->mode);
    if (cfg->channels != FMRX_MONO && cfg->channels != FMRX_STEREO)
        return fail(FMRX_EINVAL, "invalid channels %d", cfg->channels);
    const int rf_taps = cfg->rf_taps ? cfg->rf_taps : 51;
    const int bp_taps = cfg->bp_taps ? cfg->bp_taps : 51;
    const int audio_taps = cfg->audio_taps ? cfg->audio_taps : 51;
    if (rf_taps < 3 || rf_taps > kMaxRfTaps) return fail(FMRX_EINVAL, "rf_taps %d out of range", rf_taps);
    if (bp_taps < 3 || bp_taps > 64) return fail(FMRX_EINVAL, "bp_taps %d out of range", bp_taps);
    // The fused audio stages (mono window, rational resampler rows, stereo LPFs' shared
    // 50-sample history) are compiled for the reference's 51 taps per phase (project.cpp:319).
    if (audio_taps != 51) return fail(FMRX_EINVAL, "audio_taps %d unsupported (51 per phase)", audio_taps);
    g->rf_fs = m.rf_fs;
    g->rf_decim = m.rf_decim;
    g->if_fs = m.if_fs;
    g->bp_fs = m.bp_fs;
    g->audio_up = m.audio_up;
    g->audio_down = m.audio_down;
    g->rf_taps = rf_taps;
    g->bp_taps = bp_taps;
    g->audio_taps_total = audio_taps * m.audio_up;  // project.cpp:347,356
    g->block_bytes = (size_t)256 * m.rf_decim * m.audio_down;  // project.cpp:364
    g->iq_pairs = g->block_bytes / 2;
    g->if_samples = g->iq_pairs / m.rf_decim;
    g->audio_frames = g->if_samples * m.audio_up / m.audio_down;
    g->pcm_samples = g->audio_frames * cfg->channels;
    if ((size_t)g->audio_taps_total - 1 > g->if_samples || (size_t)rf_taps - 1 > g->iq_pairs)
        return fail(FMRX_EINVAL, "filter longer than a block");
    return FMRX_OK;
}

// The tuning switches of a new context from the environment (A/B measurements: which runner or
// kernel form runs, never what it computes).  The PLL test hooks are not read here: only
// fmrx_debug_set_knob sets them, per context.
// Every knob's accepted range (include/fmrx.h): a value outside it is refused (FMRX_EINVAL from
// fmrx_debug_set_knob; fmrx_create refuses a bad environment variable), so no setting can reach
// an untested kernel form.  Integer knobs take integer values only.
struct KnobSpec {
    int id;
    const char* env;  // the tuning knobs' environment variable (null: test hooks, never from there)
    double lo, hi;
    bool integer;
};
constexpr KnobSpec kKnobs[] = {
    {FMRX_KNOB_PLL_SPEC, "FMRX_PLL_SPEC", 0, 1, true},
    {FMRX_KNOB_PLL_SAT, "FMRX_PLL_SAT", 0, 1, true},
    {FMRX_KNOB_PLL_PRED, "FMRX_PLL_PRED", 0, 2, true},
    {FMRX_KNOB_PLL_PIPE, "FMRX_PLL_PIPE", 0, 1, true},
    {FMRX_KNOB_PLL_IDX, "FMRX_PLL_IDX", 0, 2, true},
    {FMRX_KNOB_STEREO_CHUNKS, "FMRX_STEREO_CHUNKS", 0, 64, true},
    {FMRX_KNOB_MONO_SPLIT, "FMRX_MONO_SPLIT", -1, 1023, true},
    {FMRX_KNOB_BPF_TILE, "FMRX_BPF_TILE", 0, 1, true},
    {FMRX_KNOB_HALO_KERNEL, "FMRX_HALO_KERNEL", 0, 1, true},
    {FMRX_KNOB_PLL_INJECT, nullptr, -1, 1 << 30, true},
    {FMRX_KNOB_PLL_PIPE_MISS, nullptr, -(1 << 30), 1 << 30, true},
    {FMRX_KNOB_PLL_HINT_SKEW, nullptr, -16777216.0, 16777216.0, false},
    {FMRX_KNOB_PLL_CNT, "FMRX_PLL_CNT", 0, 31, true},
    {FMRX_KNOB_PLL_STICK, "FMRX_PLL_STICK", 0, 1, true},
    {FMRX_KNOB_STEREO_HEAD, "FMRX_STEREO_HEAD", 1, 64, true},
    {FMRX_KNOB_STEREO_LEAD, "FMRX_STEREO_LEAD", 0, 64, true},
    {FMRX_KNOB_AUDIO_DEFER, "FMRX_AUDIO_DEFER", 0, 64, true},
    {FMRX_KNOB_STEREO_TAIL, "FMRX_STEREO_TAIL", 1, 64, true},
};

const KnobSpec* knob_spec(int knob) {
    for (const KnobSpec& k : kKnobs)
        if (k.id == knob) return &k;
    return nullptr;
}

// value into the context's knobs (range already checked)
void knob_set(fmrx_ctx::Knobs& k, int knob, double value) {
    const int v = (int)value;
    switch (knob) {
        case FMRX_KNOB_PLL_SPEC: k.pll.spec = v; break;
        case FMRX_KNOB_PLL_SAT: k.pll.sat = v; break;
        case FMRX_KNOB_PLL_PRED: k.pll.pred = v; break;
        case FMRX_KNOB_PLL_PIPE: k.pll.pipe = v; break;
        case FMRX_KNOB_PLL_IDX: k.pll.idx = v; break;
        case FMRX_KNOB_STEREO_CHUNKS: k.stereo_chunks = v; break;
        case FMRX_KNOB_STEREO_HEAD: k.stereo_head = v; break;
        case FMRX_KNOB_STEREO_TAIL: k.stereo_tail = v; break;
        case FMRX_KNOB_STEREO_LEAD: k.stereo_lead = v; break;
        case FMRX_KNOB_AUDIO_DEFER: k.audio_defer = v; break;
        case FMRX_KNOB_MONO_SPLIT: k.mono_split = v; break;
        case FMRX_KNOB_BPF_TILE: k.bpf_tile = v; break;
        case FMRX_KNOB_HALO_KERNEL: k.halo_kernel = v; break;
        case FMRX_KNOB_PLL_INJECT: k.pll.inject = v; break;
        case FMRX_KNOB_PLL_PIPE_MISS: k.pll.pipe_miss = v; break;
        case FMRX_KNOB_PLL_HINT_SKEW: k.pll.skew = value; break;
        case FMRX_KNOB_PLL_CNT: k.pll.cnt = v; break;
        case FMRX_KNOB_PLL_STICK: k.pll.stick = v; break;
        default: break;
    }
}

bool knob_ok(const KnobSpec& s, double v) {
    return v == v && v >= s.lo && v <= s.hi && (!s.integer || v == std::floor(v));
}

// the tuning knobs from the environment, read once by fmrx_create; a set variable must be an
// integer in its knob's range (otherwise the context is refused, naming the variable)
int knobs_from_env(fmrx_ctx::Knobs* out) {
    fmrx_ctx::Knobs k;
    for (const KnobSpec& s : kKnobs) {
        if (!s.env) continue;
        const char* e = std::getenv(s.env);
        if (!e || !*e) continue;
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (*end != '\0' || !knob_ok(s, (double)v))
            return fail(FMRX_EINVAL, "%s=%s: not an integer in [%g, %g]", s.env, e, s.lo, s.hi);
        knob_set(k, s.id, (double)v);
    }
    *out = k;
    return FMRX_OK;
}

int fmrx_create(const fmrx_config* cfg, fmrx_ctx** out) {
    if (!out) return fail(FMRX_EINVAL, "null output pointer");
    *out = nullptr;
    fmrx_geometry_t g;
    int rc = fmrx_geometry(cfg, &g);
    if (rc) return rc;
    if (cfg->n_streams < 1) return fail(FMRX_EINVAL, "n_streams must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(FMRX_EHIP, "no HIP device available (libfmrx has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(FMRX_EINVAL, "bad device %d", cfg->device);
    // every per-stream launch puts the streams on grid.y (band-pass, PLL check / NCO / pre-pass,
    // halo update, the multi-stream audio and copy kernels): refuse what cannot launch here
    // rather than fail at the first call
    int max_y = 0;
    if (hipDeviceGetAttribute(&max_y, hipDeviceAttributeMaxGridDimY, cfg->device) == hipSuccess && max_y > 0 &&
        cfg->n_streams > max_y)
        return fail(FMRX_EINVAL, "n_streams %d exceeds the device's grid.y limit %d", cfg->n_streams, max_y);
    fmrx_ctx* c = new fmrx_ctx();
    auto failed = [&](int code) { fmrx_destroy(c); return code; };  // the one failure path from here on
    c->cfg = *cfg;
    c->cfg.rf_taps = g.rf_taps;
    c->cfg.bp_taps = g.bp_taps;
    c->geo = g;
    if (!fused_rf_supported(c))
        return failed(fail(FMRX_EINVAL, "no compiled RF kernel for rf_taps=%d rf_decim=%d", g.rf_taps, g.rf_decim));
    if ((rc = set_device(c)) || (rc = knobs_from_env(&c->knobs))) return failed(rc);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0)
        c->n_simd = 4 * cus;
    // the context stream at the highest priority (the serial PLL of the pipelined stereo engine
    // runs on it, its stage streams at the lowest)
    int prio_lo = 0, prio_hi = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess ||
        hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi) != hipSuccess)
        return failed(fail(FMRX_EHIP, "hipStreamCreate failed"));
    init_frames(c);
    init_blend(c);
    if ((rc = init_front(c)) || (rc = init_audio(c)) || (rc = init_rds_front(c)) || (rc = init_rds_bits(c)) ||
        (rc = reset_state(c)))
        return failed(rc);
    *out = c;
    return FMRX_OK;
}

// Every buffer and event of the context frees itself when `delete` runs the members' destructors, so the
// order here is the invariant: the device is set before anything is freed, and every stream that may
// still read a buffer is synchronised before the first one goes.  The events are destroyed with their
// holders after the streams; all of them have completed by then.
void fmrx_destroy(fmrx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    for (hipStream_t s : {c->stream, c->stereo.s_front, c->stereo.s_audio})
        if (s) (void)hipStreamSynchronize(s);
    for (hipStream_t s : {c->stereo.s_front, c->stereo.s_audio, c->stream})
        if (s) (void)hipStreamDestroy(s);
    delete c;
}

int fmrx_history_bytes(const fmrx_ctx* c, size_t* bytes) {
    CtxLock lock_(c);
    if (!c || !bytes) return fail(FMRX_EINVAL, "null argument");
    *bytes = c->front.halo_bytes;
    return FMRX_OK;
}

// The fused kernel rebuilds every float state of the mono product from the raw bytes in the
// halo by a pre-roll chunk (mono_fused.hip), so seeking is setting the halo: the last
// halo_bytes of prev, the format's zero (0x80 for u8: x = 0.0, the reference's zero-initialised
// state) in front of a shorter prev.  Bytes are the context's format's (fmrx_set_input_format).
int fmrx_seek(fmrx_ctx* c, const uint8_t* prev, size_t n, int prev_on_device) {
    CtxLock lock_(c);
    if (!c || (!prev && n > 0)) return fail(FMRX_EINVAL, "bad argument");
    if (c->cfg.channels != FMRX_MONO) return fail(FMRX_ESTATE, "fmrx_seek: mono product only (the PLL is serial)");
    if (c->wide.ratio.on()) return fail(FMRX_ESTATE, "fmrx_seek: not with a capture decimation (the wide stage has no seek)");
    if (c->deemph.tau) return fail(FMRX_ESTATE, "fmrx_seek: not with de-emphasis on (its carry has no seek)");
    if (refuse_row_stages(c, "fmrx_seek", "its carry has no seek", "its carries have no seek")) return FMRX_ESTATE;
    if (n % c->front.pair_bytes != 0)
        return fail(FMRX_EINVAL, "fmrx_seek: %zu bytes are no whole number of %zu-byte I/Q pairs", n, c->front.pair_bytes);
    int rc = set_device(c);
    if (rc) return rc;
    const size_t ns = c->cfg.n_streams, hb = c->front.halo_bytes, m = std::min(n, hb);
    uint8_t* h = c->front.halo.cur();
    if (m < hb) HIPCHK(hipMemset2DAsync(h, hb, iq_zero_byte(c), hb - m, ns, c->stream));
    if (m > 0)
        HIPCHK(hipMemcpy2DAsync(h + (hb - m), hb, prev + (n - m), n, m, ns,
                                prev_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    if (!prev_on_device) HIPCHK(hipStreamSynchronize(c->stream));  // prev may be freed on return
    c->mono.stale = true;
    return FMRX_OK;
}

int fmrx_reset(fmrx_ctx* c) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    int rc = set_device(c);
    return rc ? rc : reset_state(c);
}

// ---- FM de-emphasis: configuration and a carry of its own --------------------------------------
int fmrx_set_deemphasis(fmrx_ctx* c, int tau_us) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (tau_us != 0 && tau_us != 50 && tau_us != 75)
        return fail(FMRX_EINVAL, "de-emphasis of %d us: 0 (off), 50 or 75", tau_us);
    int rc = set_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));  // a call in flight still reads the carry
    if (tau_us) {
        const size_t rows = (size_t)c->cfg.n_streams * (size_t)c->cfg.channels;
        if ((rc = ensure_deemph_taps(c)) || (rc = c->deemph.state.ensure(rows * kDeemphHist))) return rc;
    }
    c->deemph.tau = tau_us;
    if ((rc = reset_deemph(c))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

int fmrx_deemphasis(const fmrx_ctx* c, int* tau_us) {
    CtxLock lock_(c);
    if (!c || !tau_us) return fail(FMRX_EINVAL, "null argument");
    *tau_us = c->deemph.tau;
    return FMRX_OK;
}

// ---- state blob: header + halo bytes + audio history + stereo state ------------------
int fmrx_state_size(const fmrx_ctx* c, size_t* bytes) {
    CtxLock lock_(c);
    if (!c || !bytes) return fail(FMRX_EINVAL, "null argument");
    const size_t ns = c->cfg.n_streams;
    *bytes = kStateHdrWords * sizeof(uint32_t) + ns * (c->front.halo_bytes + sizeof(float) * (c->mono.hist_len + kDemodHist + 8 + kMixTail + 8));
    return FMRX_OK;
}

namespace {
struct BlobIO {
    uint8_t* p;
    bool put;
    int io(fmrx_ctx* c, void* dev, size_t n) {
        if (n == 0) return 0;
        if (put) HIPCHK(hipMemcpyAsync(dev, p, n, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(hipMemcpyAsync(p, dev, n, hipMemcpyDeviceToHost, c->stream));
        p += n;
        return 0;
    }
};

int state_io(fmrx_ctx* c, uint8_t* buf, size_t bytes, bool put) {
    size_t need;
    fmrx_state_size(c, &need);
    if (bytes < need) return fail(FMRX_ESTATE, "state buffer too small (%zu < %zu)", bytes, need);
    int rc = set_device(c);
    if (rc) return rc;
    // words 0-7 identify the context shape and must match; word 8 carries the audio-history
    // staleness of a context taken between fmrx_seek and its next fused call (bit 0; restored with
    // the blob, so fmrx_audio_block refuses the stale history there too) and the raw I/Q format
    // (bits 8-15), which must match
    uint32_t hdr[kStateHdrWords] = {kStateMagic, kStateVersion, (uint32_t)c->cfg.mode, (uint32_t)c->cfg.channels,
                                    (uint32_t)c->geo.rf_taps, (uint32_t)c->cfg.n_streams, (uint32_t)c->front.halo_bytes,
                                    (uint32_t)c->mono.hist_len,
                                    (c->mono.stale ? 1u : 0u) | ((uint32_t)c->front.format << 8), 0u};
    if (put) {
        uint32_t got[kStateHdrWords];
        std::memcpy(got, buf, sizeof got);
        if (got[0] != kStateMagic) return fail(FMRX_ESTATE, "not an fmrx state blob (magic 0x%08x)", got[0]);
        if (got[1] != kStateVersion)
            return fail(FMRX_ESTATE, "state blob version %u, expected %u (INTEGRATION.md: blob versions)", got[1],
                        kStateVersion);
        // word 8, bits 8-15: the raw I/Q format of the halo bytes (0 = u8: the blobs from before the
        // bits had a meaning carry 0 there and stay valid); checked before the shape, whose halo word
        // the format changes
        if ((got[8] & ~0xFF01u) == 0u && (got[8] >> 8) != (uint32_t)c->front.format)
            return fail(FMRX_ESTATE, "state blob holds input format %u, the context is set to %d", got[8] >> 8,
                        c->front.format);
        if (std::memcmp(hdr + 2, got + 2, 6 * sizeof(uint32_t)) != 0)
            return fail(FMRX_ESTATE, "state blob is for another context shape (mode %u, channels %u, rf_taps %u, "
                        "%u streams)", got[2], got[3], got[4], got[5]);
        if ((got[8] & ~0xFF01u) != 0u) return fail(FMRX_ESTATE, "state blob: unknown flags 0x%x", got[8]);
        if (got[9] != 0u) return fail(FMRX_ESTATE, "state blob: reserved word 9 is 0x%x, must be 0", got[9]);
    } else {
        std::memcpy(buf, hdr, sizeof hdr);
    }
    const size_t ns = c->cfg.n_streams;
    if ((rc = ensure_demod(c, 1))) return rc;  // rows that hold the history at least
    BlobIO b{buf + sizeof hdr, put};
    if ((rc = b.io(c, c->front.halo.cur(), ns * c->front.halo_bytes))) return rc;
    if ((rc = b.io(c, c->mono.hist.p, ns * sizeof(float) * c->mono.hist_len))) return rc;
    // demod history: kDemodHist floats in front of each stream's row (one 2-D copy)
    {
        const size_t w = sizeof(float) * kDemodHist, pitch = sizeof(float) * c->stereo.demod_stride;
        if (put) HIPCHK(hipMemcpy2DAsync(c->stereo.demod.p, pitch, b.p, w, w, ns, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(hipMemcpy2DAsync(b.p, w, c->stereo.demod.p, pitch, w, ns, hipMemcpyDeviceToHost, c->stream));
        b.p += w * ns;
    }
    if ((rc = b.io(c, c->stereo.pll.p, ns * sizeof(float) * 8))) return rc;
    // (slots 6-7 of each stream's PLL state are the runners' hand-off within a call, 0 between
    // calls: a blob's values there are not trusted)
    if (put)
        HIPCHK(hipMemset2DAsync(c->stereo.pll.p + 6, 8 * sizeof(float), 0, 2 * sizeof(float), ns, c->stream));
    if ((rc = b.io(c, c->stereo.mix_tail.p, ns * sizeof(float) * kMixTail))) return rc;
    if ((rc = b.io(c, c->stereo.mono_state.p, ns * sizeof(float) * 8))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
}  // namespace

int fmrx_get_state(fmrx_ctx* c, void* buf, size_t bytes) {
    CtxLock lock_(c);
    if (!c || !buf) return fail(FMRX_EINVAL, "null argument");
    if (c->wide.ratio.on()) return fail(FMRX_ESTATE, "fmrx_get_state: not with a capture decimation (no checkpoint of the wide stage)");
    if (c->deemph.tau) return fail(FMRX_ESTATE, "fmrx_get_state: not with de-emphasis on (the blob does not hold its carry)");
    if (refuse_row_stages(c, "fmrx_get_state", "the blob does not hold its carry", "the blob does not hold its carries")) return FMRX_ESTATE;
    return state_io(c, static_cast<uint8_t*>(buf), bytes, false);
}

int fmrx_set_state(fmrx_ctx* c, const void* buf, size_t bytes) {
    CtxLock lock_(c);
    if (!c || !buf) return fail(FMRX_EINVAL, "null argument");
    if (c->wide.ratio.on()) return fail(FMRX_ESTATE, "fmrx_set_state: not with a capture decimation (no checkpoint of the wide stage)");
    if (c->deemph.tau) return fail(FMRX_ESTATE, "fmrx_set_state: not with de-emphasis on (the blob does not hold its carry)");
    if (refuse_row_stages(c, "fmrx_set_state", "the blob does not hold its carry", "the blob does not hold its carries")) return FMRX_ESTATE;
    const uint8_t* p = static_cast<const uint8_t*>(buf);
    const int rc = state_io(c, const_cast<uint8_t*>(p), bytes, true);
    if (rc == 0) {
        uint32_t flags;
        std::memcpy(&flags, p + 8 * sizeof(uint32_t), sizeof flags);
        c->mono.stale = (flags & 1u) != 0;
        // the streams' trigOffsets (state_io order: halo, audio history, demod history, PLL x 8)
        const size_t ns = c->cfg.n_streams;
        const uint8_t* pll = p + kStateHdrWords * sizeof(uint32_t) +
                             ns * (c->front.halo_bytes + sizeof(float) * (c->mono.hist_len + kDemodHist));
        TrigTrack t;
        t.lo = 16777216.0;
        t.hi = 0.0;
        for (size_t s = 0; s < ns; s++) {
            float v;
            std::memcpy(&v, pll + (8 * s + 5) * sizeof(float), sizeof v);
            if (!(v >= 0.0f && v <= 16777216.0f && v == std::floor(v))) t.known = false;
            t.lo = std::min(t.lo, (double)v);
            t.hi = std::max(t.hi, (double)v);
        }
        if (!t.known) t.lo = t.hi = 0.0;
        c->stereo.trig = t;
    }
    return rc;
}

int fmrx_synchronize(fmrx_ctx* c) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        // an asynchronous fault of an enqueued launch: the device state no longer follows the
        // host's trigOffset bounds, so the runner choice falls back to "unknown" until a reset
        c->stereo.trig.known = false;
        c->rds.trig.known = false;
        return fail(FMRX_EHIP, "stream synchronize failed: %s", hipGetErrorString(e));
    }
    return FMRX_OK;
}

void* fmrx_stream(fmrx_ctx* c) { return c ? (void*)c->stream : nullptr; }

int fmrx_kernel_timing(fmrx_ctx* c, int reset, double* avg_ms, long* launches) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    int rc = set_device(c);
    if (rc) return rc;
    double total = 0.0;
    if (c->diag.ev_used) HIPCHK(hipEventSynchronize(c->diag.evs[c->diag.ev_used - 1].second));
    for (size_t i = 0; i < c->diag.ev_used; i++) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, c->diag.evs[i].first, c->diag.evs[i].second));
        total += ms;
    }
    if (avg_ms) *avg_ms = c->diag.ev_used ? total / (double)c->diag.ev_used : 0.0;
    if (launches) *launches = (long)c->diag.ev_used;
    if (reset) {  // reset > 0: clear and arm event timing of the fused kernel; reset < 0: clear and disarm
        c->diag.ev_used = 0;
        c->diag.timing = reset > 0;
    }
    return FMRX_OK;
}

// Diagnostic: per-stage device time of the stereo engine (StageTimer).  op 1 arms (and clears),
// 0 reads, -1 reads and disarms; the read waits for the last recorded event.
int fmrx_debug_stage_timing(fmrx_ctx* c, int op, double* ms, double* steps, long* launches, int n_kinds) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    int rc = set_device(c);
    if (rc) return rc;
    StageTimer& T = c->diag.timer;
    if (op == 1) {
        T.on = true;
        T.used = 0;
        return FMRX_OK;
    }
    if (n_kinds < 0 || (n_kinds > 0 && (!ms || !steps || !launches))) return fail(FMRX_EINVAL, "bad argument");
    for (int k = 0; k < n_kinds; k++) {
        ms[k] = steps[k] = 0.0;
        launches[k] = 0;
    }
    if (T.used) HIPCHK(hipEventSynchronize(T.recs[T.used - 1].b));
    for (size_t i = 0; i < T.used; i++) {
        const StageTimer::Rec& r = T.recs[i];
        if (r.kind >= n_kinds) continue;
        float t = 0.0f;
        HIPCHK(hipEventSynchronize(r.b));
        HIPCHK(hipEventElapsedTime(&t, r.a, r.b));
        ms[r.kind] += t;
        steps[r.kind] += r.steps;
        launches[r.kind] += 1;
    }
    if (op == -1) {
        T.on = false;
        T.used = 0;
    }
    return FMRX_OK;
}

int fmrx_debug_set_knob(fmrx_ctx* c, int knob, double value) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    const KnobSpec* s = knob_spec(knob);
    if (!s) return fail(FMRX_EINVAL, "unknown knob %d", knob);
    if (!knob_ok(*s, value)) return fail(FMRX_EINVAL, "knob %d: %g outside [%g, %g]", knob, value, s->lo, s->hi);
    knob_set(c->knobs, knob, value);
    return FMRX_OK;
}

}  // extern "C"
