// engine.cpp — the launch sequences behind the entry points: the fused RF front end, the mono audio
// stage, the stereo engine (serial and pipelined) and the RDS front half, on the context's streams.
#include "ctx.h"

namespace fmrx {

// RDS front half over n_if new demod samples per stream (d_demod: ns x n_if, stride
// demod_stride).  Optional copies of the NCO and the channel (ns x n_if each).
int run_rds(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_if, float* d_out,
            float* d_nco, float* d_channel) {
    const int ns = c->cfg.n_streams;
    if (kRdsChanHist + n_if > c->rds_chan_stride) {
        const size_t stride = kRdsChanHist + n_if;
        DevBuf<float> nb;
        int rc = nb.ensure(stride * ns);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(nb.p, 0, sizeof(float) * nb.n, c->stream));
        if (c->d_rds_chan.p) {
            HIPCHK(hipMemcpy2DAsync(nb.p, stride * sizeof(float), c->d_rds_chan.p,
                                    c->rds_chan_stride * sizeof(float), kRdsChanHist * sizeof(float), ns,
                                    hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            c->d_rds_chan.release();
        }
        c->d_rds_chan = nb;
        c->rds_chan_stride = stride;
    }
    int rc = c->d_rds_car.ensure(n_if * ns);
    if (!rc) rc = c->d_pll_side.ensure(pll_side_doubles((int)n_if, ns));
    if (rc) return rc;
    RdsLaunch L{};
    L.demod = d_demod;
    L.demod_stride = demod_stride;
    L.dhist = c->d_rds_dhist.p;
    L.chan = c->d_rds_chan.p;
    L.chan_stride = c->rds_chan_stride;
    L.carrier = c->d_rds_car.p;
    L.car_stride = n_if;
    L.out = d_out;
    L.out_stride = n_if;
    L.pll = c->d_rds_pll.p;
    L.pll_side = c->d_pll_side.p;
    L.ex = c->d_rds_taps.p;
    L.ca = c->d_rds_taps.p + kRdsTaps;
    L.bp_fs = (float)c->geo.bp_fs;
    L.n_if = (int)n_if;
    L.hint = c->hint(c->rds_trig);
    L.hint.redos = nullptr;  // fmrx_debug_pll_redos counts the stereo PLL's streams only
    if (launch_rds(L, ns, c->stream)) {
        c->rds_trig.known = false;
        return fail(FMRX_EHIP, "RDS launch failed");
    }
    c->rds_trig.advance(n_if);
    if (d_nco)
        HIPCHK(hipMemcpyAsync(d_nco, c->d_rds_car.p, sizeof(float) * n_if * ns, hipMemcpyDeviceToDevice,
                              c->stream));
    if (d_channel)
        HIPCHK(hipMemcpy2DAsync(d_channel, n_if * sizeof(float), c->d_rds_chan.p + kRdsChanHist,
                                c->rds_chan_stride * sizeof(float), n_if * sizeof(float), ns,
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

}  // namespace

// ---- de-emphasis behind the audio stages (deemph.hip) ------------------------------
int ensure_deemph_taps(fmrx_ctx* c) {
    if (c->d_deemph_taps.p) return 0;
    float h[2 * kDeemphTaps];
    if (!deemph_design(deemph_audio_fs(c), 50, h) || !deemph_design(deemph_audio_fs(c), 75, h + kDeemphTaps))
        return fail(FMRX_EINVAL, "no de-emphasis design at %d S/s", deemph_audio_fs(c));
    int rc = c->d_deemph_taps.ensure(2 * kDeemphTaps);
    if (rc) return rc;
    HIPCHK(hipMemcpy(c->d_deemph_taps.p, h, sizeof h, hipMemcpyHostToDevice));
    return 0;
}

int deemph_rows(fmrx_ctx* c, size_t na, float* d_mono, float** rows) {
    if (c->cfg.channels == FMRX_MONO && d_mono) {
        *rows = d_mono;
        return 0;
    }
    const int rc = c->d_deemph_x.ensure((size_t)c->cfg.n_streams * na * (size_t)c->cfg.channels);
    *rows = c->d_deemph_x.p;
    return rc;
}

int run_deemph(fmrx_ctx* c, const float* rows, size_t na, int16_t* d_pcm) {
    DeemphLaunch D{};
    D.in = rows;
    D.nch = c->cfg.channels == FMRX_MONO ? 1 : 2;
    D.in_stride = na * (size_t)D.nch;
    D.n = na;
    D.h = c->d_deemph_taps.p + (c->deemph_tau == 75 ? kDeemphTaps : 0);
    D.state_in = c->d_deemph_state[c->deemph_cur].p;
    D.state_out = c->d_deemph_state[c->deemph_cur ^ 1].p;
    D.out = nullptr;
    D.pcm = d_pcm;
    D.out_stride = D.in_stride;
    if (launch_deemph(D, c->cfg.n_streams, c->stream)) return fail(FMRX_EHIP, "de-emphasis launch failed");
    c->deemph_cur ^= 1;
    return 0;
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
    L.halo = b0 == 0 ? c->d_halo[c->halo_cur].p : d_iq + b0 * bb - c->halo_bytes;
    L.halo_stride = b0 == 0 ? c->halo_bytes : L.iq_stride;
    L.pcm = d_pcm;
    L.mono = d_mono;
    // de-emphasis on: the kernel's float outlet feeds deemph.hip, which then writes the call's PCM
    float* dx = nullptr;
    if (with_audio && c->deemph_tau) {
        const int rc_dx = deemph_rows(c, n_blocks * c->geo.audio_frames, d_mono, &dx);
        if (rc_dx) return rc_dx;
        L.mono = dx;
    }
    L.demod = d_demod ? d_demod + b0 * c->geo.if_samples : nullptr;
    L.demod_stride = demod_stride;
    L.demod_hist = demod_hist;
    // When this call produces the mono audio itself, the mono product's audio history stays in
    // step with the stream, so a later fmrx_audio_block continues from it: its last 50 samples
    // are all a resampler output reads back (51 taps per phase in every mode).  The RF-only
    // calls (fmrx_rf_block, the stereo engine) leave it alone: the audio stage they feed owns it.
    L.demod_tail = with_audio ? c->d_audio_hist.p + (c->audio_hist - kAudioHist50) : nullptr;
    L.demod_tail_stride = (size_t)c->audio_hist;
    L.audio_coeff = c->d_audio.p;
    L.audio_rows = c->d_audio_rows.p;
    L.stream_bytes = n_blocks * c->geo.block_bytes;
    L.halo_bytes = c->halo_bytes;
    L.n_if = (long long)(n_blocks * c->geo.if_samples);
    L.segs = mono_segments(c, L.n_if, b0 > 0 ? kPipeFrontWgPerCu : 0);
    L.older_share = mono_older_share(c, L.segs);
    L.stamps = c->stamps;
    L.audio = with_audio ? 1 : 0;
    // the halo update rides in the fused kernel when every stream row is 16-B aligned (halo
    // bytes and block bytes are multiples of 16); otherwise halo_kernel runs after it
    const bool fused_halo = (reinterpret_cast<uintptr_t>(L.iq) & 15) == 0 && L.stream_bytes % 16 == 0 &&
                            L.iq_stride % 16 == 0 && c->halo_bytes % 16 == 0 &&
                            c->knobs.halo_kernel != 1;  // knob halo_kernel = 1: the separate kernel (A/B)
    L.halo_next = (last && fused_halo) ? c->d_halo[c->halo_cur ^ 1].p : nullptr;
    const int ad = c->geo.audio_up == 1 ? c->geo.audio_down : 5;
    TimingPair* ev = nullptr;
    int rc = timing_begin(c, st, &ev);
    if (rc) return rc;
    const int st_t = (!with_audio && d_demod) ? c->stage_timer.begin(st) : -1;
    rc = launch_mono_fused(L, ns, c->geo.rf_taps, c->geo.rf_decim, c->geo.audio_up,
                           c->geo.audio_up == 1 ? ad : c->geo.audio_down, c->mono_taps, st);
    c->stage_timer.end(st_t, kStFront, 0.0, st);
    if (rc != 0) return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "fused kernel launch failed (%d)", rc);
    if ((rc = timing_end(ev, st))) return rc;
    if (with_audio) c->audio_hist_stale = false;  // demod_tail rewrote the audio history
    if (dx && (rc = run_deemph(c, dx, n_blocks * c->geo.audio_frames, d_pcm))) return rc;
    if (!last) return 0;
    if (!L.halo_next) {  // the whole call's tail (every chunk's bytes are in d_iq)
        rc = launch_halo_update(d_iq, call_blocks * bb, c->d_halo[c->halo_cur].p, c->d_halo[c->halo_cur ^ 1].p,
                                c->halo_bytes, ns, st);
        if (rc != 0) return fail(FMRX_EHIP, "halo update failed");
    }
    c->halo_cur ^= 1;
    return 0;
}

// Mono product audio stage on a demod buffer (generic polyphase path: modes 2/3 and the
// split API).  demod: ns x n_if contiguous.  Advances d_audio_hist.
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
    P.state = c->d_audio_hist.p;
    P.state_stride = c->audio_hist;
    P.coeff = c->d_audio.p;
    P.taps = at;
    P.up = c->geo.audio_up;
    P.down = c->geo.audio_down;
    P.n_out = (int)na;
    float* dx = nullptr;  // de-emphasis on: the float outlet feeds deemph.hip, which then writes d_pcm
    if (c->deemph_tau) {
        const int rc_dx = deemph_rows(c, na, d_mono, &dx);
        if (rc_dx) return rc_dx;
        d_mono = dx;
    }
    P.out = d_mono;
    P.out_stride = na;
    P.pcm = d_pcm;
    P.pcm_stride = na;
    int rc = launch_polyphase(P, ns, c->stream);
    if (rc == 0 && n_if >= (size_t)(at - 1))
        rc = launch_copy_streams(c->d_audio_hist.p, c->audio_hist, d_demod + (n_if - (at - 1)), demod_stride,
                                 at - 1, ns, c->stream);
    if (rc) return fail(FMRX_EHIP, "mono audio stage launch failed");
    return dx ? run_deemph(c, dx, na, d_pcm) : 0;
}

// Stereo engine on c->d_demod (history in front, n_if new samples per stream).
// src (may be null): the call's new demod, n_if a stream contiguous, not yet in c->d_demod --
// the band-pass kernel reads it from there (pinned host memory: no copy launch) and stores it.
int run_stereo_audio(fmrx_ctx* c, size_t n_blocks, int16_t* d_pcm, float* d_mono, const float* src) {
    const int ns = c->cfg.n_streams;
    const size_t n_if = n_blocks * c->geo.if_samples;
    int rc = c->d_channel.ensure(n_if * ns);
    if (!rc) rc = c->d_carrier.ensure(n_if * ns);
    if (rc) return rc;
    StereoLaunch S{};
    S.demod = c->d_demod.p;
    S.channel = c->d_channel.p;
    S.carrier = c->d_carrier.p;
    S.n_if = (int)n_if;
    S.out_stride = n_if;
    S.hist = kDemodHist;
    S.demod_stride = c->demod_stride;
    S.ch_c = c->ch.data();
    S.ca_c = c->ca.data();
    S.bp_taps = c->geo.bp_taps;
    S.src = src;
    const int t_bp = c->stage_timer.begin(c->stream);
    if (launch_bpf_pair(S, ns, c->stream, c->knobs.bpf_tile != 0)) return fail(FMRX_EHIP, "band-pass launch failed");
    c->stage_timer.end(t_bp, kStBpf, 0.0, c->stream);
    const PllLoop pilot = pilot_loop(c);
    if ((rc = c->d_pll_side.ensure(pll_side_doubles((int)n_if, ns)))) return rc;
    // a call of a few blocks (the per-block seam): the NCO, audio, state carry and demod history in
    // one launch after the PLL (launch_stereo_audio_small); longer calls: the parallel kernels
    const bool small = c->geo.audio_up == 1 && n_blocks <= (size_t)kSmallAudioBlocks;
    if (launch_pll(c->d_carrier.p, (int)n_if, ns, n_if, pilot, c->d_pll.p, c->d_pll_side.p, c->stream,
                   c->hint(c->pll_trig), c->pll_stats, !small)) {
        c->pll_trig.known = false;
        return fail(FMRX_EHIP, "PLL launch failed");
    }
    c->pll_trig.advance(n_if);
    // de-emphasis on: the audio kernels' (right, left) outlet feeds deemph.hip, which then writes d_pcm
    const size_t na = n_blocks * c->geo.audio_frames;
    float* dx = nullptr;
    if (c->deemph_tau && (rc = deemph_rows(c, na, nullptr, &dx))) return rc;
    AudioLaunch A{};
    A.demod = c->d_demod.p;
    A.demod_stride = c->demod_stride;
    A.hist = kDemodHist;
    A.channel = c->d_channel.p;
    A.nco = c->d_carrier.p;
    A.mix_tail = c->d_mix_tail.p;
    A.mono_state = c->d_mono_state.p;
    A.pcm = d_pcm;
    A.mono_out = d_mono;
    A.lr_out = reinterpret_cast<float2*>(dx);
    A.n_blocks = (int)n_blocks;
    A.if_per_block = (int)c->geo.if_samples;
    A.frames_per_block = (int)c->geo.audio_frames;
    A.up = c->geo.audio_up;
    A.down = c->geo.audio_down;
    A.at = c->geo.audio_taps_total;
    A.audio_c = c->d_audio.p;
    const int t_au = c->stage_timer.begin(c->stream);
    if (small) {
        if (launch_stereo_audio_small(A, ns, pll_scratch(c->d_pll_side.p, (int)n_if, ns).args, n_if, pilot.nco_scale,
                                      pilot.phase_adjust, c->d_pll.p, kDemodHist, c->stream))
            return fail(FMRX_EHIP, "stereo audio launch failed");
        c->stage_timer.end(t_au, kStAudio, 0.0, c->stream);
        return dx ? run_deemph(c, dx, na, d_pcm) : 0;
    }
    if (launch_stereo_audio(A, ns, c->stream)) return fail(FMRX_EHIP, "stereo audio launch failed");
    c->stage_timer.end(t_au, kStAudio, 0.0, c->stream);
    // demod history for the next call: last kDemodHist samples -> front, every stream in one
    // launch (n_if >= one block of IF samples > kDemodHist: the ranges never overlap)
    if (launch_copy_streams(c->d_demod.p, c->demod_stride, c->d_demod.p + n_if, c->demod_stride, kDemodHist, ns,
                            c->stream))
        return fail(FMRX_EHIP, "demod history copy failed");
    return dx ? run_deemph(c, dx, na, d_pcm) : 0;
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
    const size_t hb = (c->halo_bytes + c->geo.block_bytes - 1) / c->geo.block_bytes;
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
// runs the serial PLL of chunk k (launch_pll over its samples, the state carried in d_pll),
// s_front the front end and band-pass pair of chunk k + 1 ahead of it, s_audio the audio stage of
// chunk k - 1 behind it.  Every chunk reads the call's buffers (demod with its history, channel,
// carrier/NCO) at its offset, so each stage sees exactly the serial engine's inputs: the same
// bits.  Events order chunk k's PLL after its band-pass and its audio after its PLL; the call
// ends with the context stream waiting for the audio stream.
int run_stereo_pipelined(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm, float* d_mono, int K) {
    const int rc = run_stereo_pipelined_body(c, d_iq, n_blocks, d_pcm, d_mono, K);
    if (rc != 0 && c->s_front) {
        // a launch failed part-way: the context stream still waits for whatever the side streams
        // hold, so a later call (or fmrx_synchronize) never races them
        c->pll_trig.known = false;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreateWithFlags(&e0, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&e1, hipEventDisableTiming) == hipSuccess) {
            (void)hipEventRecord(e0, c->s_front);
            (void)hipEventRecord(e1, c->s_audio);
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
        if ((cb(k + 1) - cb(k)) * c->geo.block_bytes < c->halo_bytes)
            return fail(FMRX_EINVAL, "chunks shorter than the halo");
    int rc = c->d_channel.ensure(n_if * ns);
    if (!rc) rc = c->d_carrier.ensure(n_if * ns);
    if (rc) return rc;
    if (!c->s_front) {  // the lowest priority: the PLL's launches go first when a CU frees up
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&c->s_front, hipStreamNonBlocking, lo));
        HIPCHK(hipStreamCreateWithPriority(&c->s_audio, hipStreamNonBlocking, lo));
    }
    const size_t n_ev = 3 * (size_t)K + 3;
    while (c->pipe_ev.size() < n_ev) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->pipe_ev.push_back(e);
    }
    hipEvent_t ev_start = c->pipe_ev[0], ev_end = c->pipe_ev[1], ev_lane = c->pipe_ev[2 * (size_t)K + 2];
    auto ev_bp = [&](int k) { return c->pipe_ev[2 + 2 * (size_t)k]; };
    auto ev_pll = [&](int k) { return c->pipe_ev[3 + 2 * (size_t)k]; };
    auto ev_nco = [&](int k) { return c->pipe_ev[2 * (size_t)K + 3 + (size_t)k]; };
    // both side streams start after everything enqueued on the context stream so far
    HIPCHK(hipEventRecord(ev_start, c->stream));
    HIPCHK(hipStreamWaitEvent(c->s_front, ev_start, 0));
    HIPCHK(hipStreamWaitEvent(c->s_audio, ev_start, 0));
    size_t max_m = 0;
    for (int k = 0; k < K; k++)
        max_m = std::max(max_m, (cb(k + 1) - cb(k)) * ipb);
    if ((rc = c->d_pll_side.ensure(pll_side_doubles((int)max_m, ns)))) return rc;
    if ((rc = c->d_pll_side2.ensure(pll_side_doubles((int)max_m, ns)))) return rc;
    // de-emphasis on: the (right, left) outlet of every chunk's audio stage, then deemph.hip over the
    // whole call on the context stream once it has waited for the audio stream
    const size_t na = n_blocks * c->geo.audio_frames;
    float* dx = nullptr;
    if (c->deemph_tau && (rc = deemph_rows(c, na, nullptr, &dx))) return rc;
    AudioLaunch A{};
    A.demod = c->d_demod.p;
    A.demod_stride = c->demod_stride;
    A.hist = kDemodHist;
    A.channel = c->d_channel.p;
    A.nco = c->d_carrier.p;
    A.mix_tail = c->d_mix_tail.p;
    A.mono_state = c->d_mono_state.p;
    A.pcm = d_pcm;
    A.mono_out = d_mono;
    A.lr_out = reinterpret_cast<float2*>(dx);
    A.n_blocks = (int)n_blocks;
    A.if_per_block = (int)ipb;
    A.frames_per_block = (int)c->geo.audio_frames;
    A.up = c->geo.audio_up;
    A.down = c->geo.audio_down;
    A.at = c->geo.audio_taps_total;
    A.audio_c = c->d_audio.p;
    // the PLL of chunk 0 in two launches when its streams start below 2^18: the lane runner's
    // segments and the index runner's [2^17, 2^18) form first (issue-bound: a front-end wave
    // sharing a chain's SIMD halves its rate), then the rest; chunk 1's front end waits for the
    // first part
    size_t lane_m = 0;
    if (c->pll_trig.known && c->pll_trig.lo == c->pll_trig.hi && c->pll_trig.lo < (double)kPllIdxMin)
        lane_m = (size_t)((double)kPllIdxMin - c->pll_trig.lo);
    // a chunk's PLL leaves its NCO (filter.cpp:170, a parallel pass) to the audio stream, so the
    // context stream goes on to the next chunk's runners; chunk k's trigArgs stay in side buffer
    // k & 1 until that NCO has read them (the context stream waits for it before chunk k + 2)
    auto side_of = [&](int k) { return (k & 1) ? c->d_pll_side2.p : c->d_pll_side.p; };
    const PllLoop pilot = pilot_loop(c);
    auto pll = [&](size_t off, size_t m, double* side, bool nco) -> int {
        if (m == 0) return 0;
        PllHint h = c->hint(c->pll_trig);
        h.demote_once = true;  // one demoted-kernel launch a chunk (beside the stage kernels)
        if (launch_pll(c->d_carrier.p + off, (int)m, ns, n_if, pilot, c->d_pll.p, side, c->stream, h, c->pll_stats, nco)) {
            c->pll_trig.known = false;
            return fail(FMRX_EHIP, "PLL launch failed");
        }
        c->pll_trig.advance(m);
        return 0;
    };
    // the audio stage of chunk j (s_audio, after chunk j's NCO)
    auto audio = [&](int j) -> int {
        const int t_au = c->stage_timer.begin(c->s_audio);
        if (launch_stereo_audio_range(A, (int)cb(j), (int)cb(j + 1), j == K - 1, ns, c->s_audio))
            return fail(FMRX_EHIP, "stereo audio launch failed");
        c->stage_timer.end(t_au, kStAudio, 0.0, c->s_audio);
        return 0;
    };
    for (int k = 0; k < K; k++) {
        const size_t b0 = cb(k), b1 = cb(k + 1);
        const size_t nb = b1 - b0, m = nb * ipb, off = b0 * ipb;
        const bool last = k == K - 1;
        if (k == 1 && lane_m > 0) HIPCHK(hipStreamWaitEvent(c->s_front, ev_lane, 0));
        // paced: chunk k's front end runs beside chunk k - lead + 1's PLL, not all of them at the start
        const int lead = c->knobs.stereo_lead;
        if (lead > 0 && k >= lead) HIPCHK(hipStreamWaitEvent(c->s_front, ev_pll(k - lead), 0));
        // s_front: front end and band-pass pair of chunk k
        if ((rc = run_fused(c, d_iq, nb, nullptr, nullptr, c->d_demod.p, c->demod_stride, kDemodHist, false, b0,
                            n_blocks, c->s_front, last)))
            return rc;
        StereoLaunch S{};
        S.demod = c->d_demod.p + off;
        S.channel = c->d_channel.p + off;
        S.carrier = c->d_carrier.p + off;
        S.n_if = (int)m;
        S.out_stride = n_if;
        S.hist = kDemodHist;
        S.demod_stride = c->demod_stride;
        S.ch_c = c->ch.data();
        S.ca_c = c->ca.data();
        S.bp_taps = c->geo.bp_taps;
        const int t_bp = c->stage_timer.begin(c->s_front);
        if (launch_bpf_pair(S, ns, c->s_front, c->knobs.bpf_tile != 0)) return fail(FMRX_EHIP, "band-pass launch failed");
        c->stage_timer.end(t_bp, kStBpf, 0.0, c->s_front);
        HIPCHK(hipEventRecord(ev_bp(k), c->s_front));
        // the context stream: the PLL of chunk k (project.cpp:166)
        HIPCHK(hipStreamWaitEvent(c->stream, ev_bp(k), 0));
        if (k >= 2) HIPCHK(hipStreamWaitEvent(c->stream, ev_nco(k - 2), 0));  // side buffer k & 1 read
        const size_t m0 = k == 0 ? std::min(lane_m, m) : 0;
        if ((rc = pll(off, m0, side_of(k), true))) return rc;  // (the lane part: its NCO in place)
        if (k == 0 && lane_m > 0) HIPCHK(hipEventRecord(ev_lane, c->stream));
        if ((rc = pll(off + m0, m - m0, side_of(k), false))) return rc;
        HIPCHK(hipEventRecord(ev_pll(k), c->stream));
        // s_audio: the NCO and the audio stage of chunk k (and the state carry after the last)
        HIPCHK(hipStreamWaitEvent(c->s_audio, ev_pll(k), 0));
        const int t_nco = c->stage_timer.begin(c->s_audio);
        if (launch_pll_nco(c->d_carrier.p + off + m0, (int)(m - m0), ns, n_if, pilot, c->d_pll.p, side_of(k), c->s_audio))
            return fail(FMRX_EHIP, "NCO launch failed");
        c->stage_timer.end(t_nco, kStNco, 0.0, c->s_audio);
        HIPCHK(hipEventRecord(ev_nco(k), c->s_audio));
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
    if (launch_copy_streams(c->d_demod.p, c->demod_stride, c->d_demod.p + n_if, c->demod_stride, kDemodHist, ns,
                            c->s_audio))
        return fail(FMRX_EHIP, "demod history copy failed");
    HIPCHK(hipEventRecord(ev_end, c->s_audio));
    HIPCHK(hipStreamWaitEvent(c->stream, ev_end, 0));
    return dx ? run_deemph(c, dx, na, d_pcm) : 0;
}
}  // namespace

int ensure_demod(fmrx_ctx* c, size_t n_if) {
    const size_t stride = kDemodHist + n_if;
    if (stride <= c->demod_stride) return 0;
    // grow, preserving the history of every stream
    DevBuf<float> nb;
    int rc = nb.ensure(stride * c->cfg.n_streams);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(nb.p, 0, sizeof(float) * nb.n, c->stream));
    if (c->d_demod.p) {
        HIPCHK(hipMemcpy2DAsync(nb.p, stride * sizeof(float), c->d_demod.p,
                                c->demod_stride * sizeof(float), kDemodHist * sizeof(float),
                                c->cfg.n_streams, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->d_demod.release();
    }
    c->d_demod = nb;
    c->demod_stride = stride;
    return 0;
}

}  // namespace fmrx
