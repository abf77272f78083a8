// process.cpp — the block-streaming entry points: the device-resident calls, the host-buffer calls
// with their staging, and the split per-stage calls of the reference's threads (rf, audio, RDS).
#include <chrono>
#include <cstring>

#include "ctx.h"

using namespace fmrx;

namespace {

int check_wide_tuned(const fmrx_ctx* c, const char* who) {
    if (!c->wide.ratio.on() || !c->wide.tuned)
        return fail(FMRX_ESTATE, "%s: wide tuning is off (fmrx_set_capture_decim, fmrx_tune_wide first)", who);
    return 0;
}

// End of a small host call: poll the stream instead of hipStreamSynchronize, whose blocking wait
// wakes the thread ~10 us after the last kernel of a 20-80 us call (the per-block seam's
// calls); after kSpinNs the call is not small after all and blocks.
constexpr long long kSpinNs = 2000000;
int wait_small(fmrx_ctx* c) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0;; k++) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e == hipSuccess) return FMRX_OK;
        if (e != hipErrorNotReady) return fail(FMRX_EHIP, "stream query: %s", hipGetErrorString(e));
        if ((k & 63) == 63 && std::chrono::duration_cast<std::chrono::nanoseconds>(
                                  std::chrono::steady_clock::now() - t0).count() > kSpinNs)
            break;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

// A host call's input to the device and its out_n results of type T back.  enqueue(src, res, pinned)
// puts the call's work on the context stream: it reads src and writes res.
// The route: a call of up to kPinnedCallBytes input bytes, where `pinned_ok`, is staged through the
// pinned buffers -- the input copied into h_in, the results written by the kernels into h_out in
// place, then a polling wait and one host copy; any other call reads the caller's buffer, writes
// `d_res` and copies that back on the stream, then a blocking wait.
// src: with `upload`, d_in, filled from the staged input by DMA; without, the staged input itself
// (h_in, or the caller's pageable buffer), which enqueue then brings to the device as it sees fit.
template <class T, class Enqueue>
int staged_call(fmrx_ctx* c, const void* in, size_t in_bytes, bool upload, DevBuf<T>& d_res, T* out, size_t out_n,
                bool pinned_ok, Enqueue enqueue) {
    const bool pinned = pinned_ok && in_bytes <= kPinnedCallBytes;
    int rc;
    if (pinned && ((rc = c->io.h_in.ensure(in_bytes)) || (rc = c->io.h_out.ensure(out_n * sizeof(T))))) return rc;
    if (upload && (rc = c->io.d_in.ensure(in_bytes))) return rc;
    if (!pinned && (rc = d_res.ensure(out_n))) return rc;
    const void* src = in;
    if (pinned) {
        std::memcpy(c->io.h_in.p, in, in_bytes);
        src = c->io.h_in.p;
    }
    if (upload) {
        HIPCHK(hipMemcpyAsync(c->io.d_in.p, src, in_bytes, hipMemcpyHostToDevice, c->stream));
        src = c->io.d_in.p;
    }
    T* res = pinned ? reinterpret_cast<T*>(c->io.h_out.p) : d_res.p;
    if ((rc = enqueue(src, res, pinned))) return rc;
    if (pinned) {
        if ((rc = wait_small(c))) return rc;
        std::memcpy(out, res, out_n * sizeof(T));
        return FMRX_OK;
    }
    HIPCHK(hipMemcpyAsync(out, res, out_n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

// shared (fmrx_process_shared): iq is one stream's bytes, read by every (tuned) stream
int process_host(fmrx_ctx* c, const uint8_t* iq, size_t n_blocks, int16_t* pcm, bool shared) {
    CtxLock lock_(c);
    if (!c || !iq || !pcm) return fail(FMRX_EINVAL, "null argument");
    if (shared && !c->tune.on) return fail(FMRX_ESTATE, "fmrx_process_shared: tuning is off (fmrx_tune first)");
    if (n_blocks == 0) return FMRX_OK;
    int rc = front_tuned(c) ? 0 : refuse_row_stages(c, "an untuned call", "the fused path writes no demod rows; fmrx_tune with zero offsets first");
    if (rc || (rc = set_device(c))) return rc;
    if ((rc = check_call_size(c, n_blocks))) return rc;
    const size_t ns = c->cfg.n_streams;
    const size_t in_bytes = (shared ? 1 : ns) * n_blocks * iq_block_bytes(c);
    auto on_device = shared ? fmrx_process_shared_device : fmrx_process_device;
    return staged_call(c, iq, in_bytes, true, c->io.d_out, pcm, ns * n_blocks * c->geo.pcm_samples, true,
                       [&](const void* d_iq, int16_t* d_pcm, bool) {
                           return on_device(c, static_cast<const uint8_t*>(d_iq), n_blocks, d_pcm);
                       });
}

}  // namespace

extern "C" {

// ---- fused device-resident path ----------------------------------------------------------
int fmrx_process_device_ex(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm,
                           float* d_mono) {
    CtxLock lock_(c);
    if (!c || !d_iq || !d_pcm) return fail(FMRX_EINVAL, "null argument");
    if (n_blocks == 0) return FMRX_OK;
    int rc = set_device(c);
    if (rc) return rc;
    if (front_tuned(c)) {
        if ((rc = check_call_size(c, n_blocks))) return rc;
        return run_tuned(c, d_iq, n_blocks * iq_block_bytes(c), n_blocks, d_pcm, d_mono);
    }
    if ((rc = refuse_row_stages(c, "an untuned call", "the fused path writes no demod rows; fmrx_tune with zero offsets first"))) return rc;
    const size_t n_if = n_blocks * c->geo.if_samples;
    if (c->cfg.channels == FMRX_MONO)  // every mode: RF + demod + audio resampler in one launch
        return run_fused(c, d_iq, n_blocks, d_pcm, d_mono, nullptr, 0, 0, true);
    if ((rc = ensure_demod(c, n_if))) return rc;
    const int K = stereo_chunks(c, n_blocks);
    if (K > 1) return run_stereo_pipelined(c, d_iq, n_blocks, d_pcm, d_mono, K);
    if ((rc = run_fused(c, d_iq, n_blocks, nullptr, nullptr, c->stereo.demod.p, c->stereo.demod_stride,
                        kDemodHist, false)))
        return rc;
    return run_stereo_audio(c, n_blocks, d_pcm, d_mono);
}

int fmrx_process_device(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm) {
    return fmrx_process_device_ex(c, d_iq, n_blocks, d_pcm, nullptr);
}

int fmrx_process_shared_device(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm) {
    CtxLock lock_(c);
    if (!c || !d_iq || !d_pcm) return fail(FMRX_EINVAL, "null argument");
    if (!c->tune.on) return fail(FMRX_ESTATE, "fmrx_process_shared_device: tuning is off (fmrx_tune first)");
    if (n_blocks == 0) return FMRX_OK;
    int rc = set_device(c);
    if (rc) return rc;
    return run_tuned(c, d_iq, 0, n_blocks, d_pcm, nullptr);
}

int fmrx_process_wide_device(fmrx_ctx* c, const uint8_t* d_iq, size_t n_blocks, int16_t* d_pcm) {
    CtxLock lock_(c);
    if (!c || !d_iq || !d_pcm) return fail(FMRX_EINVAL, "null argument");
    int rc = check_wide_tuned(c, "fmrx_process_wide_device");
    if (rc) return rc;
    if (n_blocks == 0) return FMRX_OK;
    if (reinterpret_cast<uintptr_t>(d_iq) % (2 * c->front.pair_bytes) != 0)
        return fail(FMRX_EINVAL, "wide calls need a %zu-byte aligned capture", 2 * c->front.pair_bytes);
    if ((rc = check_wide_blocks(c, n_blocks)) || (rc = check_call_size(c, n_blocks, c->wide.ratio.size_factor())) || (rc = set_device(c)))
        return rc;
    return run_wide(c, d_iq, n_blocks, d_pcm);
}

// ---- host-buffer entry points ---------------------------------------------------------------
int fmrx_process(fmrx_ctx* c, const uint8_t* iq, size_t n_blocks, int16_t* pcm) {
    return process_host(c, iq, n_blocks, pcm, false);
}

int fmrx_process_shared(fmrx_ctx* c, const uint8_t* iq, size_t n_blocks, int16_t* pcm) {
    return process_host(c, iq, n_blocks, pcm, true);
}

// one wide capture (n_blocks * decim * iq_pairs pairs) read by every stream; device buffers at every size
int fmrx_process_wide(fmrx_ctx* c, const uint8_t* iq, size_t n_blocks, int16_t* pcm) {
    CtxLock lock_(c);
    if (!c || !iq || !pcm) return fail(FMRX_EINVAL, "null argument");
    int rc = check_wide_tuned(c, "fmrx_process_wide");
    if (rc) return rc;
    if (n_blocks == 0) return FMRX_OK;
    if ((rc = set_device(c))) return rc;
    if ((rc = check_wide_blocks(c, n_blocks)) || (rc = check_call_size(c, n_blocks, c->wide.ratio.size_factor()))) return rc;
    const size_t in_bytes = wide_pairs_of(c, n_blocks) * c->front.pair_bytes;
    const size_t out_n = (size_t)c->cfg.n_streams * n_blocks * c->geo.pcm_samples;
    return staged_call(c, iq, in_bytes, true, c->io.d_out, pcm, out_n, false, [&](const void* d_iq, int16_t* d_pcm, bool) {
        return fmrx_process_wide_device(c, static_cast<const uint8_t*>(d_iq), n_blocks, d_pcm);
    });
}

// rf_thread body (project.cpp:48-70): u8 blocks -> demod floats.
int fmrx_rf_block(fmrx_ctx* c, const uint8_t* iq, size_t n_blocks, float* demod) {
    CtxLock lock_(c);
    if (!c || !iq || !demod) return fail(FMRX_EINVAL, "null argument");
    if (n_blocks == 0) return FMRX_OK;
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = check_call_size(c, n_blocks))) return rc;
    const size_t ns = c->cfg.n_streams;
    const size_t n_if = n_blocks * c->geo.if_samples;
    // pinned staging: the input by DMA (the fused kernel's staging reads host memory 4x slower),
    // the demod in place
    return staged_call(c, iq, ns * n_blocks * iq_block_bytes(c), true, c->io.f32, demod, ns * n_if, true,
                       [&](const void* src, float* d_demod, bool) {
                           const uint8_t* d_iq = static_cast<const uint8_t*>(src);
                           return front_tuned(c) ? run_tuned_front(c, d_iq, n_blocks * iq_block_bytes(c), n_blocks,
                                                                   d_demod, n_if, 0, false)
                                                 : run_fused(c, d_iq, n_blocks, nullptr, nullptr, d_demod, n_if, 0, false);
                       });
}

// audio_thread body (project.cpp:132-195): demod floats -> S16.
int fmrx_audio_block(fmrx_ctx* c, const float* demod, size_t n_blocks, int16_t* pcm) {
    CtxLock lock_(c);
    if (!c || !demod || !pcm) return fail(FMRX_EINVAL, "null argument");
    if (n_blocks == 0) return FMRX_OK;
    int rc = refuse_row_stages(c, "fmrx_audio_block", "the stage runs in the tuned calls");
    if (rc || (rc = set_device(c))) return rc;
    const size_t ns = c->cfg.n_streams;
    const size_t n_if = n_blocks * c->geo.if_samples;
    if (c->cfg.channels == FMRX_MONO && c->mono.stale)
        return fail(FMRX_ESTATE, "no audio history after fmrx_seek (run a fused call first)");
    // small calls: the demod through the pinned staging (stereo: read there by the band-pass
    // kernel; mono: one copy), the PCM written by the audio kernel into pinned memory in place
    auto audio = [&](const void* staged, int16_t* d_pcm, bool pinned) {
        const float* src = static_cast<const float*>(staged);
        int rc;
        if (c->cfg.channels == FMRX_MONO) {
            if ((rc = c->io.f32.ensure(ns * n_if))) return rc;
            HIPCHK(hipMemcpyAsync(c->io.f32.p, src, sizeof(float) * ns * n_if, hipMemcpyHostToDevice, c->stream));
            return run_mono_audio(c, c->io.f32.p, n_if, n_if, d_pcm, nullptr);
        }
        if ((rc = ensure_demod(c, n_if))) return rc;
        if (!pinned)
            HIPCHK(hipMemcpy2DAsync(c->stereo.demod.p + kDemodHist, c->stereo.demod_stride * sizeof(float), src,
                                    n_if * sizeof(float), n_if * sizeof(float), ns,
                                    hipMemcpyHostToDevice, c->stream));
        // pinned: the band-pass kernel reads the staging buffer itself (one launch fewer)
        return run_stereo_audio(c, n_blocks, d_pcm, nullptr, pinned ? src : nullptr);
    };
    return staged_call(c, demod, sizeof(float) * ns * n_if, false, c->io.d_out, pcm, ns * n_blocks * c->geo.pcm_samples, true,
                       audio);
}

// ---- RDS front half (rds_thread body, project.cpp:200-271) -------------------------------
int fmrx_rds_block(fmrx_ctx* c, const float* demod, size_t n_blocks, float* rds, float* nco,
                   float* channel) {
    CtxLock lock_(c);
    if (!c || !demod || !rds) return fail(FMRX_EINVAL, "null argument");
    if (n_blocks == 0) return FMRX_OK;
    int rc = set_device(c);
    if (rc) return rc;
    const size_t ns = c->cfg.n_streams;
    const size_t n = ns * n_blocks * c->geo.if_samples;
    if ((rc = c->io.f32.ensure(n)) || (rc = c->io.scratch.ensure(3 * n))) return rc;
    float* d_rds = c->io.scratch.p;
    float* d_nco = nco ? c->io.scratch.p + n : nullptr;
    float* d_ch = channel ? c->io.scratch.p + 2 * n : nullptr;
    HIPCHK(hipMemcpyAsync(c->io.f32.p, demod, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_rds(c, c->io.f32.p, n / ns, n / ns, d_rds, d_nco, d_ch))) return rc;
    HIPCHK(hipMemcpyAsync(rds, d_rds, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    if (nco) HIPCHK(hipMemcpyAsync(nco, d_nco, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    if (channel) HIPCHK(hipMemcpyAsync(channel, d_ch, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

int fmrx_rds_device(fmrx_ctx* c, const float* d_demod, size_t n_blocks, float* d_rds, float* d_nco,
                    float* d_channel) {
    CtxLock lock_(c);
    if (!c || !d_demod || !d_rds) return fail(FMRX_EINVAL, "null argument");
    if (n_blocks == 0) return FMRX_OK;
    int rc = set_device(c);
    if (rc) return rc;
    const size_t n_if = n_blocks * c->geo.if_samples;
    return run_rds(c, d_demod, n_if, n_if, d_rds, d_nco, d_channel);
}

}  // extern "C"
