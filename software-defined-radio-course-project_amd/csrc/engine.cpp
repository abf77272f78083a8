// engine.cpp — the launch sequences behind the entry points: the fused RF front end, the mono audio
// stage, the stereo engine (serial and pipelined) and the RDS front half, on the context's streams.
#include "ctx.h"

namespace fmrx {

// The rows of `buf` (n_streams of `stride` floats) grown to new_stride a stream, zero but for the first
// `hist` floats of every row, which are kept; the context stream is drained before the old rows go
static int grow_rows(fmrx_ctx* c, DevBuf<float>& buf, size_t& stride, size_t hist, size_t new_stride) {
    if (new_stride <= stride) return 0;
    const int ns = c->cfg.n_streams;
    DevBuf<float> nb;
    int rc = nb.ensure(new_stride * ns);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(nb.p, 0, sizeof(float) * nb.n, c->stream));
    if (buf.p) {
        HIPCHK(hipMemcpy2DAsync(nb.p, new_stride * sizeof(float), buf.p, stride * sizeof(float), hist * sizeof(float), ns,
                                hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        buf.release();
    }
    buf = std::move(nb);
    stride = new_stride;
    return 0;
}

// The audio stages at creation: the taps exactly as the reference designs them (project.cpp:37, 97, 104,
// 117) and their device copies, the sine table, the mono history and the stereo engine's carried state.
int init_audio(fmrx_ctx* c) {
    const fmrx_geometry_t& g = c->geo;
    const size_t ns = c->cfg.n_streams;
    auto& t = c->taps;
    t.rf.resize(g.rf_taps);
    design_lpf(t.rf.data(), (float)g.rf_fs, (float)kRfFc, g.rf_taps, 1);
    t.audio.resize(g.audio_taps_total);
    design_lpf(t.audio.data(), (float)g.if_fs, (float)kAudioFc, g.audio_taps_total, g.audio_up);
    t.ch.resize(g.bp_taps);
    design_bpf(t.ch.data(), (float)g.bp_fs, 22000.0f, 54000.0f, g.bp_taps);
    t.ca.resize(g.bp_taps);
    design_bpf(t.ca.data(), (float)g.bp_fs, 18500.0f, 19500.0f, g.bp_taps);
    std::copy(t.rf.begin(), t.rf.end(), t.mono.rf);
    if (g.audio_up == 1) std::copy(t.audio.begin(), t.audio.end(), t.mono.audio);
    c->mono.hist_len = g.audio_taps_total - 1;
    int rc;
    if ((rc = c->mono.hist.ensure((size_t)c->mono.hist_len * ns)) || (rc = c->stereo.pll.ensure(8 * ns)) ||
        (rc = c->stereo.mix_tail.ensure((size_t)kMixTail * ns)) || (rc = c->stereo.mono_state.ensure(8 * ns)) ||
        (rc = upload(t.d_audio, t.audio.data(), t.audio.size(), "tap upload")) ||
        (rc = upload(t.d_rf, t.rf.data(), t.rf.size(), "tap upload")) ||
        (rc = upload(c->synth.sintab, synth_sintab(), (size_t)kSinSize, "tap upload")))
        return rc;
    if (g.audio_up == 1) return 0;
    // the rational resampler's prototype by phase: row k0 holds the 51 taps an output of
    // phase k0 reads, in the order filter.cpp:84 visits them (k = k0, k0 + up, ...)
    const int up = g.audio_up;
    std::vector<float> rows((size_t)up * kAudioRow, 0.0f);
    for (int k0 = 0; k0 < up; k0++)
        for (int i = 0; i < 51; i++) rows[(size_t)k0 * kAudioRow + i] = t.audio[(size_t)k0 + (size_t)i * up];
    return upload(t.d_audio_rows, rows.data(), rows.size(), "tap upload");
}

// Zero histories and the PLL at its start; every call overwrites the demod rows past their history
int reset_audio(fmrx_ctx* c, const std::vector<float>& pll0) {
    const size_t ns = c->cfg.n_streams;
    auto& S = c->stereo;
    S.trig = TrigTrack{};
    HIPCHK(hipMemsetAsync(c->mono.hist.p, 0, sizeof(float) * c->mono.hist_len * ns, c->stream));
    c->mono.stale = false;
    if (S.demod.p)
        HIPCHK(hipMemset2DAsync(S.demod.p, S.demod_stride * sizeof(float), 0, sizeof(float) * kDemodHist, ns, c->stream));
    HIPCHK(hipMemcpyAsync(S.pll.p, pll0.data(), sizeof(float) * pll0.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(S.mix_tail.p, 0, sizeof(float) * kMixTail * ns, c->stream));
    HIPCHK(hipMemsetAsync(S.mono_state.p, 0, sizeof(float) * 8 * ns, c->stream));
    return 0;
}

// RDS taps, project.cpp:211 and :217 (bp_taps = 51 at bp_fs)
int init_rds_front(fmrx_ctx* c) {
    const size_t ns = c->cfg.n_streams;
    std::vector<float> taps(2 * kRdsTaps);
    design_bpf(taps.data(), (float)c->geo.bp_fs, 54000.0f, 60000.0f, kRdsTaps);
    design_bpf(taps.data() + kRdsTaps, (float)c->geo.bp_fs, 113500.0f, 114500.0f, kRdsTaps);
    int rc = c->rds.dhist.ensure((size_t)kRdsDemodHist * ns);
    if (!rc) rc = c->rds.pll.ensure(8 * ns);
    return rc ? rc : upload(c->rds.taps, taps.data(), taps.size(), "RDS tap upload");
}

int reset_rds_front(fmrx_ctx* c, const std::vector<float>& pll0) {
    auto& R = c->rds;
    R.trig = TrigTrack{};
    HIPCHK(hipMemsetAsync(R.dhist.p, 0, sizeof(float) * R.dhist.n, c->stream));
    if (R.chan.p) HIPCHK(hipMemsetAsync(R.chan.p, 0, sizeof(float) * R.chan.n, c->stream));
    HIPCHK(hipMemcpyAsync(R.pll.p, pll0.data(), sizeof(float) * pll0.size(), hipMemcpyHostToDevice, c->stream));
    return 0;
}

// RDS front half over n_if new demod samples per stream (d_demod: ns x n_if, stride
// demod_stride).  Optional copies of the NCO and the channel (ns x n_if each).
int run_rds(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_if, float* d_out,
            float* d_nco, float* d_channel) {
    const int ns = c->cfg.n_streams;
    int rc = grow_rows(c, c->rds.chan, c->rds.chan_stride, kRdsChanHist, kRdsChanHist + n_if);
    if (!rc) rc = c->rds.car.ensure(n_if * ns);
    if (!rc) rc = c->stereo.pll_side.ensure(pll_side_doubles((int)n_if, ns));
    if (rc) return rc;
    RdsLaunch L{};
    L.demod = d_demod;
    L.demod_stride = demod_stride;
    L.dhist = c->rds.dhist.p;
    L.chan = c->rds.chan.p;
    L.chan_stride = c->rds.chan_stride;
    L.carrier = c->rds.car.p;
    L.car_stride = n_if;
    L.out = d_out;
    L.out_stride = n_if;
    L.pll = c->rds.pll.p;
    L.pll_side = c->stereo.pll_side.p;
    L.ex = c->rds.taps.p;
    L.ca = c->rds.taps.p + kRdsTaps;
    L.bp_fs = (float)c->geo.bp_fs;
    L.n_if = (int)n_if;
    L.hint = c->hint(c->rds.trig);
    L.hint.redos = nullptr;  // fmrx_debug_pll_redos counts the stereo PLL's streams only
    if (launch_rds(L, ns, c->stream)) {
        c->rds.trig.known = false;
        return fail(FMRX_EHIP, "RDS launch failed");
    }
    c->rds.trig.advance(n_if);
    if (d_nco)
        HIPCHK(hipMemcpyAsync(d_nco, c->rds.car.p, sizeof(float) * n_if * ns, hipMemcpyDeviceToDevice,
                              c->stream));
    if (d_channel)
        HIPCHK(hipMemcpy2DAsync(d_channel, n_if * sizeof(float), c->rds.chan.p + kRdsChanHist,
                                c->rds.chan_stride * sizeof(float), n_if * sizeof(float), ns,
                                hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

namespace {

// stereo calls of up to this many blocks a stream take launch_stereo_audio_small (modes 0/1)
constexpr int kSmallAudioBlocks = 4;

// project.cpp:166: PLL(carrier, 19000, if_fs, 2, 0, 0.01, ...), the stereo pilot's loop
PllLoop pilot_loop(const fmrx_ctx* c) { return PllLoop{19000.0f, (float)c->geo.if_fs, 2.0f, 0.0f, 0.01f}; }

// Segments per stream for the fused kernel: enough workgroups to fill the chip
// (2 resident per CU on 256 CUs) without making segments so short that the pre-roll chunk
// dominates.
int mono_segments(const fmrx_ctx* c, long long n_if, int wg_per_cu = 0) {
    const long long chunks = mono_chunks(n_if, c->geo.rf_taps, c->geo.rf_decim, c->geo.audio_down);
    // one full wave of workgroups (or wg_per_cu a CU: the pipelined stereo front end, which
    // leaves the rest of each CU's LDS and SIMDs to the PLL runners beside it)
    const long long target_wg = 256LL * (wg_per_cu > 0 ? wg_per_cu : mono_wg_per_cu(c->geo.rf_decim));
    long long segs = std::max<long long>(1, target_wg / std::max(1, c->cfg.n_streams));
    // a call too short to fill the grid even at one chunk a segment (the per-block seam: 4-5
    // chunks a stream) takes one chunk a segment: twice the chunks, but all of them at once
    if ((long long)c->cfg.n_streams * chunks <= target_wg) return (int)std::max<long long>(1, chunks);
    segs = std::min(segs, std::max<long long>(1, chunks / 4));
    return (int)std::max<long long>(1, segs);
}

// Unequal shares for the two waves of a SIMD (mono_fused.hip mono_share): when the grid is
// two resident waves per SIMD (segs even, >= 15/16 of 2 x the SIMD count, 8 workgroups per
// CU), the first-dispatched wave takes kOlderShare/1024 of each span.  Knob mono_split = n
// (FMRX_MONO_SPLIT at creation) overrides it (0 = equal segments; timing sweeps).  660 since round 3's latency cuts (sweeps of
// 580-700 on two boxes, profiles/r03/split_sweep*/: 660 fastest on both, 1.2-1.6 % ahead of 620).
constexpr int kOlderShare = 660;
int mono_older_share(const fmrx_ctx* c, int segs) {
    const int n_simd = c->n_simd;
    const int share = c->knobs.mono_split < 0 ? kOlderShare : c->knobs.mono_split;
    if (share <= 0 || share >= 1024) return 0;
    const long long wgs = (long long)segs * c->cfg.n_streams;
    if ((segs & 1) != 0 || mono_wg_per_cu(c->geo.rf_decim) != 8 || wgs * 16 < 2LL * n_simd * 15 || wgs > 2LL * n_simd)
        return 0;
    return share;
}

// Workgroups a CU of the pipelined stereo front end past the first chunk (two of the fused
// kernel's 18.8 KB and one wave each): a full grid (8 a CU) holds every CU's LDS for its whole
// span, and a PLL launch queued behind it on the context stream waits until it drains.  The first
// chunk's front end runs alone (full grid).
constexpr int kPipeFrontWgPerCu = 2;

// The band-pass pair over m samples a stream at offset `off` of a call of n_if (src: run_stereo_audio's)
StereoLaunch bpf_launch(const fmrx_ctx* c, size_t off, size_t m, size_t n_if, const float* src) {
    StereoLaunch S{};
    S.demod = c->stereo.demod.p + off;
    S.channel = c->stereo.channel.p + off;
    S.carrier = c->stereo.carrier.p + off;
    S.n_if = (int)m;
    S.out_stride = n_if;
    S.hist = kDemodHist;
    S.demod_stride = c->stereo.demod_stride;
    S.ch_c = c->taps.ch.data();
    S.ca_c = c->taps.ca.data();
    S.bp_taps = c->geo.bp_taps;
    S.src = src;
    return S;
}

// The stereo audio stage over a call of n_blocks blocks a stream (lr: the de-emphasis outlet, or null)
AudioLaunch audio_launch(const fmrx_ctx* c, size_t n_blocks, int16_t* d_pcm, float* d_mono, float* lr) {
    AudioLaunch A{};
    A.demod = c->stereo.demod.p;
    A.demod_stride = c->stereo.demod_stride;
    A.hist = kDemodHist;
    A.channel = c->stereo.channel.p;
    A.nco = c->stereo.carrier.p;
    A.mix_tail = c->stereo.mix_tail.p;
    A.mono_state = c->stereo.mono_state.p;
    A.pcm = d_pcm;
    A.mono_out = d_mono;
    A.lr_out = reinterpret_cast<float2*>(lr);
    A.n_blocks = (int)n_blocks;
    A.if_per_block = (int)c->geo.if_samples;
    A.frames_per_block = (int)c->geo.audio_frames;
    A.up = c->geo.audio_up;
    A.down = c->geo.audio_down;
    A.at = c->geo.audio_taps_total;
    A.audio_c = c->taps.d_audio.p;
    return A;
}

}  // namespace

// ---- de-emphasis behind the audio stages (deemph.hip) ------------------------------
int ensure_deemph_taps(fmrx_ctx* c) {
    if (c->deemph.taps.p) return 0;
    float h[2 * kDeemphTaps];
    if (!deemph_design(deemph_audio_fs(c), 50, h) || !deemph_design(deemph_audio_fs(c), 75, h + kDeemphTaps))
        return fail(FMRX_EINVAL, "no de-emphasis design at %d S/s", deemph_audio_fs(c));
    int rc = c->deemph.taps.ensure(2 * kDeemphTaps);
    if (rc) return rc;
    HIPCHK(hipMemcpy(c->deemph.taps.p, h, sizeof h, hipMemcpyHostToDevice));
    return 0;
}

// The de-emphasis carry back to 63 zeros in front of every row (nothing to do before it was ever on)
int reset_deemph(fmrx_ctx* c) {
    PingPong<float>& st = c->deemph.state;
    st.rewind();
    if (st.cur()) HIPCHK(hipMemsetAsync(st.cur(), 0, sizeof(float) * st.buf[0].n, c->stream));
    return 0;
}

// The floats in front of the quantiser, one route for the stages that work on them: soft stereo
// (blend.hip, stereo contexts), quieting (quiet.hip) and then de-emphasis (deemph.hip).  quant_rows: where an
// audio stage's float outlet writes a call of na frames a stream while any of them is on (null while all are
// off) -- the caller's d_mono when a mono call gave one, else the context's scratch, grown to the call.
// run_quant_rows: those rows through the stages that are on into d_pcm on the context stream, the carries
// moved: soft stereo's apply kernel in place on the scratch when a stage follows, writing the PCM itself
// otherwise; quieting's from the rows into a scratch of its own when de-emphasis follows, else into the PCM.
static int quant_rows(fmrx_ctx* c, size_t na, float* d_mono, float** rows) {
    *rows = nullptr;
    if (!c->deemph.tau && !c->blend.on && !c->quiet.on) return 0;
    const size_t count = (size_t)c->cfg.n_streams * na * (size_t)c->cfg.channels;
    int rc = c->quiet.on && c->deemph.tau ? c->quiet.x.ensure(count) : 0;  // quieting's outlet when de-emphasis follows
    if (rc) return rc;
    if (c->cfg.channels == FMRX_MONO && d_mono) {
        *rows = d_mono;
        return 0;
    }
    rc = c->deemph.x.ensure(count);
    *rows = c->deemph.x.p;
    return rc;
}

static int run_deemph(fmrx_ctx* c, const float* rows, size_t na, int16_t* d_pcm) {
    DeemphLaunch D{};
    D.in = rows;
    D.nch = c->cfg.channels == FMRX_MONO ? 1 : 2;
    D.in_stride = na * (size_t)D.nch;
    D.n = na;
    D.h = c->deemph.taps.p + (c->deemph.tau == 75 ? kDeemphTaps : 0);
    D.state_in = c->deemph.state.cur();
    D.state_out = c->deemph.state.next();
    D.out = nullptr;
    D.pcm = d_pcm;
    D.out_stride = D.in_stride;
    if (launch_deemph(D, c->cfg.n_streams, c->stream)) return fail(FMRX_EHIP, "de-emphasis launch failed");
    c->deemph.state.flip();
    return 0;
}

static int run_quant_rows(fmrx_ctx* c, float* rows, size_t na, int16_t* d_pcm) {
    const bool more = c->deemph.tau != 0 || c->quiet.on;  // a stage behind soft stereo
    if (c->blend.on) {
        const int rc = blend_apply(c, rows, na, more, d_pcm);
        if (rc || !more) return rc;
    }
    const float* src = rows;
    if (c->quiet.on) {  // never in place: the rows may be a caller's d_mono
        const int rc = quiet_apply(c, rows, na, c->deemph.tau ? c->quiet.x.p : nullptr, c->deemph.tau ? nullptr : d_pcm);
        if (rc || !c->deemph.tau) return rc;
        src = c->quiet.x.p;
    }
    return run_deemph(c, src, na, d_pcm);
}

// RF front end (+ the mono audio stage when `pcm` is non-null and the mode allows it).
// Chunk form (the stereo pipeline, run_stereo_pipelined): blocks [b0, b0 + n_blocks) of a call of
// call_blocks blocks a stream starting at d_iq, on stream `st`; the halo of a chunk past the first
// is the call's own bytes in front of it, and only the last chunk (`last`) moves the context's halo.
int run_fused(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm, float* d_mono,
              float* d_demod, size_t demod_stride, int demod_hist, bool with_audio, size_t b0,
              size_t call_blocks, hipStream_t st, bool last) {
    const int ns = c->cfg.n_streams;
    const size_t bb = c->geo.block_bytes;
    if (call_blocks == 0) call_blocks = n_blocks;
    if (!st) st = c->stream;
    MonoLaunch L{};
    L.iq = d_iq + b0 * bb;
    L.iq_stride = call_blocks * bb;
    L.halo = b0 == 0 ? c->front.halo.cur() : d_iq + b0 * bb - c->front.halo_bytes;
    L.halo_stride = b0 == 0 ? c->front.halo_bytes : L.iq_stride;
    L.pcm = d_pcm;
    L.mono = d_mono;
    // de-emphasis on: the kernel's float outlet feeds deemph.hip, which then writes the call's PCM
    float* dx = nullptr;
    int rc = with_audio ? quant_rows(c, n_blocks * c->geo.audio_frames, d_mono, &dx) : 0;
    if (rc) return rc;
    if (dx) L.mono = dx;
    L.demod = d_demod ? d_demod + b0 * c->geo.if_samples : nullptr;
    L.demod_stride = demod_stride;
    L.demod_hist = demod_hist;
    // When this call produces the mono audio itself, the mono product's audio history stays in
    // step with the stream, so a later fmrx_audio_block continues from it: its last 50 samples
    // are all a resampler output reads back (51 taps per phase in every mode).  The RF-only
    // calls (fmrx_rf_block, the stereo engine) leave it alone: the audio stage they feed owns it.
    L.demod_tail = with_audio ? c->mono.hist.p + (c->mono.hist_len - kAudioHist50) : nullptr;
    L.demod_tail_stride = (size_t)c->mono.hist_len;
    L.audio_coeff = c->taps.d_audio.p;
    L.audio_rows = c->taps.d_audio_rows.p;
    L.stream_bytes = n_blocks * c->geo.block_bytes;
    L.halo_bytes = c->front.halo_bytes;
    L.n_if = (long long)(n_blocks * c->geo.if_samples);
    L.segs = mono_segments(c, L.n_if, b0 > 0 ? kPipeFrontWgPerCu : 0);
    L.older_share = mono_older_share(c, L.segs);
    L.stamps = c->diag.stamps;
    L.audio = with_audio ? 1 : 0;
    // the halo update rides in the fused kernel when every stream row is 16-B aligned (halo
    // bytes and block bytes are multiples of 16); otherwise halo_kernel runs after it
    const bool fused_halo = (reinterpret_cast<uintptr_t>(L.iq) & 15) == 0 && L.stream_bytes % 16 == 0 &&
                            L.iq_stride % 16 == 0 && c->front.halo_bytes % 16 == 0 &&
                            c->knobs.halo_kernel != 1;  // knob halo_kernel = 1: the separate kernel (A/B)
    L.halo_next = (last && fused_halo) ? c->front.halo.next() : nullptr;
    TimingPair* ev = nullptr;
    if ((rc = timing_begin(c, st, &ev))) return rc;
    const int st_t = (!with_audio && d_demod) ? c->diag.timer.begin(st) : -1;
    rc = launch_mono_fused(L, ns, c->geo.rf_taps, c->geo.rf_decim, c->geo.audio_up, c->geo.audio_down, c->taps.mono, st);
    c->diag.timer.end(st_t, kStFront, 0.0, st);
    if (rc != 0) return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "fused kernel launch failed (%d)", rc);
    if ((rc = timing_end(ev, st))) return rc;
    if (with_audio) c->mono.stale = false;  // demod_tail rewrote the audio history
    if (dx && (rc = run_quant_rows(c, dx, n_blocks * c->geo.audio_frames, d_pcm))) return rc;
    if (!last) return 0;
    if (!L.halo_next) {  // the whole call's tail (every chunk's bytes are in d_iq)
        rc = launch_halo_update(d_iq, call_blocks * bb, c->front.halo.cur(), c->front.halo.next(),
                                c->front.halo_bytes, ns, st);
        if (rc != 0) return fail(FMRX_EHIP, "halo update failed");
    }
    c->front.halo.flip();
    return 0;
}

// Mono product audio stage on a demod buffer (generic polyphase path: modes 2/3 and the
// split API).  demod: ns x n_if contiguous.  Advances mono.hist.
int run_mono_audio(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_if,
                   int16_t* d_pcm, float* d_mono) {
    const int ns = c->cfg.n_streams;
    const int at = c->geo.audio_taps_total;
    const size_t na = n_if * c->geo.audio_up / c->geo.audio_down;
    // every stream in one launch: the resampler (+ the quantiser) over (output, stream), then
    // the history move of every stream (after all reads of the old history)
    PolyStreams P{};
    P.in = d_demod;
    P.in_stride = demod_stride;
    P.state = c->mono.hist.p;
    P.state_stride = c->mono.hist_len;
    P.coeff = c->taps.d_audio.p;
    P.taps = at;
    P.up = c->geo.audio_up;
    P.down = c->geo.audio_down;
    P.n_out = (int)na;
    float* dx = nullptr;  // de-emphasis on: the float outlet feeds deemph.hip, which then writes d_pcm
    int rc = quant_rows(c, na, d_mono, &dx);
    if (rc) return rc;
    P.out = dx ? dx : d_mono;
    P.out_stride = na;
    P.pcm = d_pcm;
    P.pcm_stride = na;
    rc = launch_polyphase(P, ns, c->stream);
    if (rc == 0 && n_if >= (size_t)(at - 1))
        rc = launch_copy_streams(c->mono.hist.p, c->mono.hist_len, d_demod + (n_if - (at - 1)), demod_stride,
                                 at - 1, ns, c->stream);
    if (rc) return fail(FMRX_EHIP, "mono audio stage launch failed");
    return dx ? run_quant_rows(c, dx, na, d_pcm) : 0;
}

// Stereo engine on c->stereo.demod (history in front, n_if new samples per stream).
// src (may be null): the call's new demod, n_if a stream contiguous, not yet in c->stereo.demod --
// the band-pass kernel reads it from there (pinned host memory: no copy launch) and stores it.
int run_stereo_audio(fmrx_ctx* c, size_t n_blocks, int16_t* d_pcm, float* d_mono, const float* src) {
    const int ns = c->cfg.n_streams;
    const size_t n_if = n_blocks * c->geo.if_samples;
    int rc = c->stereo.channel.ensure(n_if * ns);
    if (!rc) rc = c->stereo.carrier.ensure(n_if * ns);
    if (rc) return rc;
    const StereoLaunch S = bpf_launch(c, 0, n_if, n_if, src);
    const int t_bp = c->diag.timer.begin(c->stream);
    if (launch_bpf_pair(S, ns, c->stream, c->knobs.bpf_tile != 0)) return fail(FMRX_EHIP, "band-pass launch failed");
    c->diag.timer.end(t_bp, kStBpf, 0.0, c->stream);
    const PllLoop pilot = pilot_loop(c);
    if ((rc = c->stereo.pll_side.ensure(pll_side_doubles((int)n_if, ns)))) return rc;
    // a call of a few blocks (the per-block seam): the NCO, audio, state carry and demod history in
    // one launch after the PLL (launch_stereo_audio_small); longer calls: the parallel kernels
    const bool small = c->geo.audio_up == 1 && n_blocks <= (size_t)kSmallAudioBlocks;
    if (launch_pll(c->stereo.carrier.p, (int)n_if, ns, n_if, pilot, c->stereo.pll.p, c->stereo.pll_side.p, c->stream,
                   c->hint(c->stereo.trig), c->diag.pll_stats, !small)) {
        c->stereo.trig.known = false;
        return fail(FMRX_EHIP, "PLL launch failed");
    }
    c->stereo.trig.advance(n_if);
    // soft stereo or de-emphasis on: the audio kernels' (right, left) outlet feeds run_quant_rows, which then writes d_pcm
    const size_t na = n_blocks * c->geo.audio_frames;
    float* dx = nullptr;
    if ((rc = quant_rows(c, na, nullptr, &dx))) return rc;
    const AudioLaunch A = audio_launch(c, n_blocks, d_pcm, d_mono, dx);
    const int t_au = c->diag.timer.begin(c->stream);
    if (small) {
        if (launch_stereo_audio_small(A, ns, pll_scratch(c->stereo.pll_side.p, (int)n_if, ns).args, n_if, pilot.nco_scale,
                                      pilot.phase_adjust, c->stereo.pll.p, kDemodHist, c->stream))
            return fail(FMRX_EHIP, "stereo audio launch failed");
        c->diag.timer.end(t_au, kStAudio, 0.0, c->stream);
        return dx ? run_quant_rows(c, dx, na, d_pcm) : 0;
    }
    if (launch_stereo_audio(A, ns, c->stream)) return fail(FMRX_EHIP, "stereo audio launch failed");
    c->diag.timer.end(t_au, kStAudio, 0.0, c->stream);
    // demod history for the next call: last kDemodHist samples -> front, every stream in one
    // launch (n_if >= one block of IF samples > kDemodHist: the ranges never overlap)
    if (launch_copy_streams(c->stereo.demod.p, c->stereo.demod_stride, c->stereo.demod.p + n_if, c->stereo.demod_stride, kDemodHist, ns,
                            c->stream))
        return fail(FMRX_EHIP, "demod history copy failed");
    return dx ? run_quant_rows(c, dx, na, d_pcm) : 0;
}

namespace {

// First block of chunk k of K (k = K: n_blocks).  The first chunk is head / 16 of the others and
// the last tail / 16 (knobs stereo_head, stereo_tail; default 8: half): the first chunk's front
// end and the last chunk's NCO and audio stage have no PLL beside them.
size_t chunk_begin(size_t n_blocks, int k, int K, int head = 8, int tail = 8) {
    if (K <= 1 || k <= 0) return k <= 0 ? 0 : n_blocks;
    if (k >= K) return n_blocks;
    const unsigned long long h = (unsigned long long)std::max(1, std::min(head, 64));
    const unsigned long long tl = (unsigned long long)std::max(1, std::min(tail, 64));
    return (size_t)(((unsigned long long)n_blocks * (h + 16ULL * (unsigned long long)(k - 1))) /
                    (h + 16ULL * (unsigned long long)(K - 2) + tl));
}

int run_stereo_pipelined_body(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm, float* d_mono,
                              int K);

}  // namespace

// Chunks of the stereo pipeline for a call of n_blocks blocks a stream: the stage work beside
// the serial PLL (front end, band-pass pair, NCO, audio) grows with the streams, the PLL's with
// the samples a stream, so a call pipelines from 16 streams on when a chunk holds enough blocks.
// Knob stereo_chunks = k (FMRX_STEREO_CHUNKS at creation) forces k chunks (1: the serial engine).
int stereo_chunks(const fmrx_ctx* c, size_t n_blocks) {
    int k = c->cfg.n_streams >= 16 ? 8 : 1;  // 32 streams x 60 s: 0.423 vs 0.430 s (profiles/r04/g9)
    if (c->knobs.stereo_chunks > 0) k = c->knobs.stereo_chunks;
    else
        while (k > 1 && n_blocks * c->geo.if_samples / (size_t)k < 16384) k--;  // >= 2^14 samples a chunk
    // a chunk past the first reads its RF halo from the call's own bytes in front of it: every
    // chunk holds at least the halo's blocks
    const size_t hb = (c->front.halo_bytes + c->geo.block_bytes - 1) / c->geo.block_bytes;
    auto short_chunk = [&](int kk) {  // a chunk of the partition shorter than the halo
        for (int j = 0; j < kk; j++)
            if (chunk_begin(n_blocks, j + 1, kk, c->knobs.stereo_head, c->knobs.stereo_tail) -
                    chunk_begin(n_blocks, j, kk, c->knobs.stereo_head, c->knobs.stereo_tail) < hb)
                return true;
        return false;
    };
    while (k > 1 && short_chunk(k)) k--;  // the short first and last chunks too
    return k;
}

// The stereo engine over the call's blocks in K chunks, pipelined like project.cpp's two threads
// and their queue (rf_thread / audio_thread, project.cpp:17,71-80,133-141): the context stream
// runs the serial PLL of chunk k (launch_pll over its samples, the state carried in stereo.pll),
// s_front the front end and band-pass pair of chunk k + 1 ahead of it, s_audio the audio stage of
// chunk k - 1 behind it.  Every chunk reads the call's buffers (demod with its history, channel,
// carrier/NCO) at its offset, so each stage sees exactly the serial engine's inputs: the same
// bits.  Events order chunk k's PLL after its band-pass and its audio after its PLL; the call
// ends with the context stream waiting for the audio stream.
int run_stereo_pipelined(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm, float* d_mono, int K) {
    const int rc = run_stereo_pipelined_body(c, d_iq, n_blocks, d_pcm, d_mono, K);
    if (rc != 0 && c->stereo.s_front) {
        // a launch failed part-way: the context stream still waits for whatever the side streams
        // hold, so a later call (or fmrx_synchronize) never races them
        c->stereo.trig.known = false;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreateWithFlags(&e0, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&e1, hipEventDisableTiming) == hipSuccess) {
            (void)hipEventRecord(e0, c->stereo.s_front);
            (void)hipEventRecord(e1, c->stereo.s_audio);
            (void)hipStreamWaitEvent(c->stream, e0, 0);
            (void)hipStreamWaitEvent(c->stream, e1, 0);
            (void)hipStreamSynchronize(c->stream);
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    return rc;
}

namespace {
int run_stereo_pipelined_body(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm, float* d_mono,
                              int K) {
    // first block of chunk j of K
    auto cb = [&](int j) { return chunk_begin(n_blocks, j, K, c->knobs.stereo_head, c->knobs.stereo_tail); };
    const int ns = c->cfg.n_streams;
    const size_t ipb = c->geo.if_samples, n_if = n_blocks * ipb;
    for (int k = 0; k < K; k++)
        if ((cb(k + 1) - cb(k)) * c->geo.block_bytes < c->front.halo_bytes)
            return fail(FMRX_EINVAL, "chunks shorter than the halo");
    int rc = c->stereo.channel.ensure(n_if * ns);
    if (!rc) rc = c->stereo.carrier.ensure(n_if * ns);
    if (rc) return rc;
    if (!c->stereo.s_front) {  // the lowest priority: the PLL's launches go first when a CU frees up
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&c->stereo.s_front, hipStreamNonBlocking, lo));
        HIPCHK(hipStreamCreateWithPriority(&c->stereo.s_audio, hipStreamNonBlocking, lo));
    }
    const size_t n_ev = 3 * (size_t)K + 3;
    while (c->stereo.pipe_ev.size() < n_ev) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->stereo.pipe_ev.push_back(e);
    }
    hipEvent_t ev_start = c->stereo.pipe_ev[0], ev_end = c->stereo.pipe_ev[1], ev_lane = c->stereo.pipe_ev[2 * (size_t)K + 2];
    auto ev_bp = [&](int k) { return c->stereo.pipe_ev[2 + 2 * (size_t)k]; };
    auto ev_pll = [&](int k) { return c->stereo.pipe_ev[3 + 2 * (size_t)k]; };
    auto ev_nco = [&](int k) { return c->stereo.pipe_ev[2 * (size_t)K + 3 + (size_t)k]; };
    // both side streams start after everything enqueued on the context stream so far
    HIPCHK(hipEventRecord(ev_start, c->stream));
    HIPCHK(hipStreamWaitEvent(c->stereo.s_front, ev_start, 0));
    HIPCHK(hipStreamWaitEvent(c->stereo.s_audio, ev_start, 0));
    size_t max_m = 0;
    for (int k = 0; k < K; k++)
        max_m = std::max(max_m, (cb(k + 1) - cb(k)) * ipb);
    if ((rc = c->stereo.pll_side.ensure(pll_side_doubles((int)max_m, ns)))) return rc;
    if ((rc = c->stereo.pll_side2.ensure(pll_side_doubles((int)max_m, ns)))) return rc;
    // de-emphasis on: the (right, left) outlet of every chunk's audio stage, then deemph.hip over the
    // whole call on the context stream once it has waited for the audio stream
    const size_t na = n_blocks * c->geo.audio_frames;
    float* dx = nullptr;
    if ((rc = quant_rows(c, na, nullptr, &dx))) return rc;
    const AudioLaunch A = audio_launch(c, n_blocks, d_pcm, d_mono, dx);
    // the PLL of chunk 0 in two launches when its streams start below 2^18: the lane runner's
    // segments and the index runner's [2^17, 2^18) form first (issue-bound: a front-end wave
    // sharing a chain's SIMD halves its rate), then the rest; chunk 1's front end waits for the
    // first part
    size_t lane_m = 0;
    if (c->stereo.trig.known && c->stereo.trig.lo == c->stereo.trig.hi && c->stereo.trig.lo < (double)kPllIdxMin)
        lane_m = (size_t)((double)kPllIdxMin - c->stereo.trig.lo);
    // a chunk's PLL leaves its NCO (filter.cpp:170, a parallel pass) to the audio stream, so the
    // context stream goes on to the next chunk's runners; chunk k's trigArgs stay in side buffer
    // k & 1 until that NCO has read them (the context stream waits for it before chunk k + 2)
    auto side_of = [&](int k) { return (k & 1) ? c->stereo.pll_side2.p : c->stereo.pll_side.p; };
    const PllLoop pilot = pilot_loop(c);
    auto pll = [&](size_t off, size_t m, double* side, bool nco) -> int {
        if (m == 0) return 0;
        PllHint h = c->hint(c->stereo.trig);
        h.demote_once = true;  // one demoted-kernel launch a chunk (beside the stage kernels)
        if (launch_pll(c->stereo.carrier.p + off, (int)m, ns, n_if, pilot, c->stereo.pll.p, side, c->stream, h, c->diag.pll_stats, nco)) {
            c->stereo.trig.known = false;
            return fail(FMRX_EHIP, "PLL launch failed");
        }
        c->stereo.trig.advance(m);
        return 0;
    };
    // the audio stage of chunk j (s_audio, after chunk j's NCO)
    auto audio = [&](int j) -> int {
        const int t_au = c->diag.timer.begin(c->stereo.s_audio);
        if (launch_stereo_audio_range(A, (int)cb(j), (int)cb(j + 1), j == K - 1, ns, c->stereo.s_audio))
            return fail(FMRX_EHIP, "stereo audio launch failed");
        c->diag.timer.end(t_au, kStAudio, 0.0, c->stereo.s_audio);
        return 0;
    };
    for (int k = 0; k < K; k++) {
        const size_t b0 = cb(k), b1 = cb(k + 1);
        const size_t nb = b1 - b0, m = nb * ipb, off = b0 * ipb;
        const bool last = k == K - 1;
        if (k == 1 && lane_m > 0) HIPCHK(hipStreamWaitEvent(c->stereo.s_front, ev_lane, 0));
        // paced: chunk k's front end runs beside chunk k - lead + 1's PLL, not all of them at the start
        const int lead = c->knobs.stereo_lead;
        if (lead > 0 && k >= lead) HIPCHK(hipStreamWaitEvent(c->stereo.s_front, ev_pll(k - lead), 0));
        // s_front: front end and band-pass pair of chunk k
        if ((rc = run_fused(c, d_iq, nb, nullptr, nullptr, c->stereo.demod.p, c->stereo.demod_stride, kDemodHist, false, b0,
                            n_blocks, c->stereo.s_front, last)))
            return rc;
        const StereoLaunch S = bpf_launch(c, off, m, n_if, nullptr);
        const int t_bp = c->diag.timer.begin(c->stereo.s_front);
        if (launch_bpf_pair(S, ns, c->stereo.s_front, c->knobs.bpf_tile != 0)) return fail(FMRX_EHIP, "band-pass launch failed");
        c->diag.timer.end(t_bp, kStBpf, 0.0, c->stereo.s_front);
        HIPCHK(hipEventRecord(ev_bp(k), c->stereo.s_front));
        // the context stream: the PLL of chunk k (project.cpp:166)
        HIPCHK(hipStreamWaitEvent(c->stream, ev_bp(k), 0));
        if (k >= 2) HIPCHK(hipStreamWaitEvent(c->stream, ev_nco(k - 2), 0));  // side buffer k & 1 read
        const size_t m0 = k == 0 ? std::min(lane_m, m) : 0;
        if ((rc = pll(off, m0, side_of(k), true))) return rc;  // (the lane part: its NCO in place)
        if (k == 0 && lane_m > 0) HIPCHK(hipEventRecord(ev_lane, c->stream));
        if ((rc = pll(off + m0, m - m0, side_of(k), false))) return rc;
        HIPCHK(hipEventRecord(ev_pll(k), c->stream));
        // s_audio: the NCO and the audio stage of chunk k (and the state carry after the last)
        HIPCHK(hipStreamWaitEvent(c->stereo.s_audio, ev_pll(k), 0));
        const int t_nco = c->diag.timer.begin(c->stereo.s_audio);
        if (launch_pll_nco(c->stereo.carrier.p + off + m0, (int)(m - m0), ns, n_if, pilot, c->stereo.pll.p, side_of(k), c->stereo.s_audio))
            return fail(FMRX_EHIP, "NCO launch failed");
        c->diag.timer.end(t_nco, kStNco, 0.0, c->stereo.s_audio);
        HIPCHK(hipEventRecord(ev_nco(k), c->stereo.s_audio));
        // audio_defer (tools/ubench_noise.hip: the audio stages' LDS tiles slow the PLL chains they
        // run beside): 0 each chunk's audio after its NCO, beside the next chunk's PLL; 1 every
        // chunk's after the last chunk's PLL (configs[4] 0.4168 -> 0.4113 s,
        // profiles/r05/ab_audio_defer/); 2, the default, chunks 0 .. K - 2 beside the LAST chunk's
        // PLL only and chunk K - 1's after it: a short tail, one chunk's chains disturbed
        // (0.4058 -> 0.3955 s, profiles/r05/ab_audio_defer2/); 2 + e, chunks 0 .. e - 1 of those
        // beside chunk K - 2's PLL instead (a shorter queue beside the last PLL).  Everything here is
        // on s_audio in issue order, so NCO(K - 1) and audio(K - 1) queue behind all deferred audio
        // stages (the intended tail); e is clamped to K - 2, so with K <= 3 the 2 + e forms are 2
        // (same bits either way: only the order on s_audio changes)
        const int ad = c->knobs.audio_defer;
        const int early = ad >= 2 ? std::min(ad - 2, K - 2) : 0;
        if (ad == 0 && (rc = audio(k))) return rc;
        if (ad >= 2 && early > 0 && k == K - 3)
            for (int j = 0; j < early; j++)
                if ((rc = audio(j))) return rc;
        if (ad >= 2 && k == K - 2)
            for (int j = early; j <= K - 2; j++)
                if ((rc = audio(j))) return rc;
        if (ad >= 2 && k == K - 1 && (rc = audio(k))) return rc;
    }
    if (c->knobs.audio_defer == 1)
        for (int j = 0; j < K; j++)
            if ((rc = audio(j))) return rc;
    // demod history for the next call (after every read of this call's demod: the last audio
    // launch follows every band-pass launch through the events)
    if (launch_copy_streams(c->stereo.demod.p, c->stereo.demod_stride, c->stereo.demod.p + n_if, c->stereo.demod_stride, kDemodHist, ns,
                            c->stereo.s_audio))
        return fail(FMRX_EHIP, "demod history copy failed");
    HIPCHK(hipEventRecord(ev_end, c->stereo.s_audio));
    HIPCHK(hipStreamWaitEvent(c->stream, ev_end, 0));
    return dx ? run_quant_rows(c, dx, na, d_pcm) : 0;
}
}  // namespace

int ensure_demod(fmrx_ctx* c, size_t n_if) {
    return grow_rows(c, c->stereo.demod, c->stereo.demod_stride, kDemodHist, kDemodHist + n_if);
}

}  // namespace fmrx
