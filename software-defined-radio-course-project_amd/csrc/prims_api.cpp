// prims_api.cpp — the reference's filter.h primitives one by one on device buffers (prims.hip), the
// synthetic input, and the diagnostic hooks that only hand a buffer to the kernels.
#include <cmath>

#include "ctx.h"

using namespace fmrx;

extern "C" {

// ---- filter.h primitives ---------------------------------------------------------------
int fmrx_impulse_response_lpf(float* h, float fs, float fc, int taps, int gain) {
    if (!h || taps < 1) return fail(FMRX_EINVAL, "bad argument");
    design_lpf(h, fs, fc, taps, gain);
    return FMRX_OK;
}

int fmrx_impulse_response_bpf(float* h, float fs, float fb, float fe, int taps) {
    if (!h || taps < 1) return fail(FMRX_EINVAL, "bad argument");
    design_bpf(h, fs, fb, fe, taps);
    return FMRX_OK;
}

int fmrx_resample(fmrx_ctx* c, float* d_out, float* d_state, const float* d_in, int n_in,
                  const float* d_coeff, int taps, int up, int down, int* n_out) {
    CtxLock lock_(c);
    if (!c || !d_out || !d_state || !d_in || !d_coeff || taps < 1 || up < 1 || down < 1)
        return fail(FMRX_EINVAL, "bad argument");
    if (n_in < taps - 1) return fail(FMRX_EINVAL, "input shorter than the filter history");
    // an output overwrites inputs that later outputs read
    if (d_out == d_in) return fail(FMRX_EINVAL, "fmrx_resample does not run in place");
    int rc = set_device(c);
    if (rc) return rc;
    const int no = (int)((long long)n_in * up / down);  // filter.cpp:77
    if (launch_resample(d_out, d_state, d_in, n_in, d_coeff, taps, up, down, no, c->stream) ||
        launch_tail_copy(d_state, d_in + (n_in - (taps - 1)), taps - 1, c->stream))
        return fail(FMRX_EHIP, "resample launch failed");
    if (n_out) *n_out = no;
    return FMRX_OK;
}

int fmrx_fm_demod(fmrx_ctx* c, float* d_out, float* d_prev, const float* d_i, const float* d_q, int n) {
    CtxLock lock_(c);
    if (!c || !d_out || !d_prev || !d_i || !d_q || n < 0) return fail(FMRX_EINVAL, "bad argument");
    // sample k reads sample k - 1 of both inputs, which another thread may have overwritten
    if (d_out == d_i || d_out == d_q) return fail(FMRX_EINVAL, "fmrx_fm_demod does not run in place");
    int rc = set_device(c);
    if (rc) return rc;
    return launch_fm_demod(d_out, d_prev, d_i, d_q, n, c->stream) ? fail(FMRX_EHIP, "launch failed") : 0;
}

int fmrx_pll(fmrx_ctx* c, float* d_io, int n, float freq, float fs, float nco_scale, float phase_adjust,
             float norm_bw, float* d_st) {
    CtxLock lock_(c);
    if (!c || !d_io || !d_st || n < 0) return fail(FMRX_EINVAL, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    // single stream with a 6-float state: stage through the 8-float layout of the kernel
    rc = c->io.scratch.ensure(8);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->io.scratch.p, d_st, 6 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    // slots 6-7 are the runners' (6: the demoted hand-off, read by every runner launch): zero
    HIPCHK(hipMemsetAsync(c->io.scratch.p + 6, 0, 2 * sizeof(float), c->stream));
    if ((rc = c->stereo.pll_side.ensure(pll_side_doubles(n, 1)))) return rc;
    // the state is the caller's: its trigOffset (read back, 4 bytes) is the hint when it is in the
    // float increments' domain (an integer in [0, 2^24]); unknown otherwise (every runner launched
    // for every segment, each taking its own streams)
    float trig = -1.0f;
    HIPCHK(hipMemcpyAsync(&trig, d_st + 5, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    TrigTrack t;
    t.known = trig >= 0.0f && trig <= 16777216.0f && trig == std::floor(trig);
    t.lo = t.hi = t.known ? (double)trig : 0.0;
    const PllHint hint = c->hint(t);  // fmrx_debug_pll_redos: as stream 0
    const PllLoop loop{freq, fs, nco_scale, phase_adjust, norm_bw};
    if (launch_pll(d_io, n, 1, (size_t)n, loop, c->io.scratch.p, c->stereo.pll_side.p, c->stream, hint, c->diag.pll_stats))
        return fail(FMRX_EHIP, "launch failed");
    HIPCHK(hipMemcpyAsync(d_st, c->io.scratch.p, 6 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return FMRX_OK;
}

int fmrx_mixer(fmrx_ctx* c, float* d_out, const float* d_a, const float* d_b, int n) {
    CtxLock lock_(c);
    if (!c || !d_out || !d_a || !d_b || n < 0) return fail(FMRX_EINVAL, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    return launch_mixer(d_out, d_a, d_b, n, c->stream) ? fail(FMRX_EHIP, "launch failed") : 0;
}

int fmrx_lr_extraction(fmrx_ctx* c, float* d_l, float* d_r, const float* d_m, const float* d_s, int n) {
    CtxLock lock_(c);
    if (!c || !d_l || !d_r || !d_m || !d_s || n < 0) return fail(FMRX_EINVAL, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    return launch_lr(d_l, d_r, d_m, d_s, n, c->stream) ? fail(FMRX_EHIP, "launch failed") : 0;
}

int fmrx_normalize_iq(fmrx_ctx* c, const uint8_t* d_iq, size_t n_pairs, float* d_i, float* d_q) {
    CtxLock lock_(c);
    if (!c || !d_iq || !d_i || !d_q) return fail(FMRX_EINVAL, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    return launch_normalize(d_iq, n_pairs, d_i, d_q, c->stream) ? fail(FMRX_EHIP, "launch failed") : 0;
}

int fmrx_quantize(fmrx_ctx* c, const float* d_x, size_t n, int16_t* d_out) {
    CtxLock lock_(c);
    if (!c || !d_x || !d_out) return fail(FMRX_EINVAL, "bad argument");
    // a 16-bit output k lies in float k / 2 of the input, which another thread reads
    if (static_cast<const void*>(d_out) == static_cast<const void*>(d_x))
        return fail(FMRX_EINVAL, "fmrx_quantize does not run in place");
    int rc = set_device(c);
    if (rc) return rc;
    return launch_quantize(d_x, n, d_out, c->stream) ? fail(FMRX_EHIP, "launch failed") : 0;
}

// ---- FM de-emphasis (no counterpart in the reference) ------------------------
int fmrx_deemph_design(int audio_fs, int tau_us, float* h64) {
    if (!h64) return fail(FMRX_EINVAL, "null tap pointer");
    if (!deemph_design(audio_fs, tau_us, h64))
        return fail(FMRX_EINVAL, "de-emphasis of %d us at %d S/s: 50 or 75 us at a positive rate", tau_us, audio_fs);
    return FMRX_OK;
}

int fmrx_deemph(fmrx_ctx* c, const float* d_in, size_t n, int tau_us, float* d_state, float* d_out, int16_t* d_pcm) {
    CtxLock lock_(c);
    if (!c || !d_in || !d_state) return fail(FMRX_EINVAL, "null argument");
    if (tau_us != 50 && tau_us != 75) return fail(FMRX_EINVAL, "de-emphasis of %d us: 50 or 75", tau_us);
    if (d_out == d_in) return fail(FMRX_EINVAL, "fmrx_deemph does not run in place");
    if (n == 0) return FMRX_OK;
    int rc = set_device(c);
    if (rc || (rc = ensure_deemph_taps(c)) || (rc = c->deemph.tmp.ensure(kDeemphHist))) return rc;
    DeemphLaunch D{};
    D.in = d_in;
    D.in_stride = n;
    D.nch = 1;
    D.n = n;
    D.h = c->deemph.taps.p + (tau_us == 75 ? kDeemphTaps : 0);
    D.state_in = d_state;
    D.state_out = c->deemph.tmp.p;  // a first chunk may still read d_state when the last one is done
    D.out = d_out;
    D.pcm = d_pcm;
    D.out_stride = n;
    if (launch_deemph(D, 1, c->stream)) return fail(FMRX_EHIP, "de-emphasis launch failed");
    HIPCHK(hipMemcpyAsync(d_state, c->deemph.tmp.p, sizeof(float) * kDeemphHist, hipMemcpyDeviceToDevice, c->stream));
    return FMRX_OK;
}

int fmrx_test_pll_fallback(fmrx_ctx* c, int kind, const float* d_a, const float* d_b, size_t n, float* d_out) {
    CtxLock lock_(c);
    if (!c || kind < 0 || kind > 2 || (n && (!d_a || !d_out || (kind == 1 && !d_b))))
        return fail(FMRX_EINVAL, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    return launch_pll_fallback_test(kind, d_a, d_b, n, d_out, c->stream) ? fail(FMRX_EHIP, "launch failed") : 0;
}

// ---- arctan demodulator ------------------------------------------------
int fmrx_fm_demod_arctan(fmrx_ctx* c, float* d_out, double* d_prev_phase, const float* d_i,
                         const float* d_q, int n) {
    CtxLock lock_(c);
    if (!c || !d_out || !d_prev_phase || !d_i || !d_q || n < 0) return fail(FMRX_EINVAL, "bad argument");
    // sample k reads sample k - 1 of both inputs, as fmrx_fm_demod
    if (d_out == d_i || d_out == d_q) return fail(FMRX_EINVAL, "fmrx_fm_demod_arctan does not run in place");
    int rc = set_device(c);
    if (rc) return rc;
    if (launch_demod_arctan(d_out, d_prev_phase, d_i, d_q, n, c->stream)) return fail(FMRX_EHIP, "launch failed");
    return FMRX_OK;
}

// ---- synthetic input --------------------------------------------------------------------
int fmrx_synth_host(uint64_t seed, int rf_fs, uint64_t first_pair, size_t n_pairs, uint8_t* out) {
    if (!out || rf_fs <= 0) return fail(FMRX_EINVAL, "bad argument");
    SynthParams p;
    synth_setup(seed, rf_fs, &p);
    const int16_t* tab = synth_sintab();
    for (size_t k = 0; k < n_pairs; k++) synth_pair(p, tab, first_pair + k, out + 2 * k);
    return FMRX_OK;
}

int fmrx_synth_device(fmrx_ctx* c, uint64_t seed, int rf_fs, uint64_t first_pair, size_t n_pairs,
                      uint8_t* d_out) {
    CtxLock lock_(c);
    if (!c || !d_out || rf_fs <= 0) return fail(FMRX_EINVAL, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    SynthParams p;
    synth_setup(seed, rf_fs, &p);
    return launch_synth(p, c->synth.sintab.p, first_pair, n_pairs, d_out, c->stream)
               ? fail(FMRX_EHIP, "synth launch failed")
               : 0;
}

int fmrx_synth_device_streams(fmrx_ctx* c, const uint64_t* seeds, size_t n_seeds, int rf_fs, uint64_t first_pair,
                              size_t n_pairs, uint8_t* d_out, size_t stride_bytes) {
    CtxLock lock_(c);
    // synth_streams_kernel stores 16-bit (I, Q) pairs at d_out + k stride: both must be even
    if (!c || !d_out || !seeds || rf_fs <= 0 || n_seeds == 0 || n_seeds > 65535 ||
        (n_seeds > 1 && stride_bytes < 2 * n_pairs) || (stride_bytes & 1) ||
        (reinterpret_cast<uintptr_t>(d_out) & 1))
        return fail(FMRX_EINVAL, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    std::vector<SynthParams> ps(n_seeds);
    for (size_t k = 0; k < n_seeds; k++) synth_setup(seeds[k], rf_fs, &ps[k]);
    if ((rc = c->synth.params.ensure(sizeof(SynthParams) * n_seeds))) return rc;
    // ps is pageable host memory: the stream is drained before it goes out of scope
    HIPCHK(hipMemcpyAsync(c->synth.params.p, ps.data(), sizeof(SynthParams) * n_seeds, hipMemcpyHostToDevice,
                          c->stream));
    if (launch_synth_streams(reinterpret_cast<const SynthParams*>(c->synth.params.p), (int)n_seeds,
                             c->synth.sintab.p, first_pair, n_pairs, d_out, stride_bytes, c->stream)) {
        (void)hipStreamSynchronize(c->stream);  // the copy from ps may still be in flight
        return fail(FMRX_EHIP, "synth launch failed");
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

// Diagnostic: per-workgroup clock stamps of the fused mono kernel (default variant, mode 0,
// 101-tap RF); the kernel's results are unchanged.  d_stamps = null turns them off.
int fmrx_debug_mono_stamps(fmrx_ctx* c, unsigned long long* d_stamps, size_t n_workgroups, size_t* needed) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    if (needed) *needed = (size_t)c->cfg.n_streams * 256 * (size_t)mono_wg_per_cu(c->geo.rf_decim);
    if (d_stamps && needed && n_workgroups < *needed)
        return fail(FMRX_EINVAL, "stamp buffer holds %zu workgroups, up to %zu launch", n_workgroups, *needed);
    c->diag.stamps = d_stamps;
    return FMRX_OK;
}

// Diagnostic: per-stream redo counts of the self-certifying PLL runners (stereo calls).
int fmrx_debug_pll_redos(fmrx_ctx* c, unsigned* d_counts) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    c->diag.pll_redos = d_counts;
    return FMRX_OK;
}

// Diagnostic: speculative-PLL counters of the stereo and PLL calls (launch_pll's spec_stats).
int fmrx_debug_pll_stats(fmrx_ctx* c, unsigned long long* d_counts) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null context");
    c->diag.pll_stats = d_counts;
    return FMRX_OK;
}

}  // extern "C"
