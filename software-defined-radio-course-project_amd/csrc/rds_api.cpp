// rds_api.cpp — the RDS back half's entry points: the bits and codes of the mixer rows
// (rds_bits.hip), the host group parser, and the decode that chains front half, bits and parser into
// the context's per-stream info.
#include <cstring>
#include <numeric>

#include "ctx.h"

using namespace fmrx;

namespace {

// bits, codes, (p, q) bytes and y of the mixer rows at d_mix (whole granules), enqueued
int run_rds_bits(fmrx_ctx* c, const float* d_mix, size_t mix_stride, size_t n_blocks, uint8_t* d_bits, uint8_t* d_codes,
                 uint8_t* d_win, float* d_y) {
    const size_t ns = c->cfg.n_streams;
    const int down = c->geo.bp_fs / 2000;
    const size_t n_if = n_blocks * c->geo.if_samples;
    if (n_if > (size_t)std::numeric_limits<int>::max() / kRdsbUp)
        return fail(FMRX_EINVAL, "%zu blocks: too many samples for one RDS call", n_blocks);
    const size_t n_out = n_if * kRdsbUp / (size_t)down, n_win = n_out / kRdsbWin, n_sym = n_win * kRdsbSyms;
    int rc = c->rdsb.work.ensure(ns * (n_out + n_sym + 2 * n_win));
    if (rc) return rc;
    RdsBitsLaunch L{};
    L.mix = d_mix;
    L.mix_stride = mix_stride;
    L.hist = c->rdsb.hist.p;
    L.state = c->rdsb.state.p;
    L.taps = c->rdsb.taps.p;
    L.sign = c->rdsb.work.p;
    L.sym = L.sign + ns * n_out;
    L.winp = L.sym + ns * n_sym;
    L.lastchip = L.winp + ns * n_win;
    L.bits = d_bits;
    L.codes = d_codes;
    L.win = d_win;
    L.y = d_y;
    L.down = down;
    L.n_if = (int)n_if;
    L.n_out = (int)n_out;
    L.n_win = (int)n_win;
    L.n_sym = (int)n_sym;
    if ((rc = launch_rds_bits(L, (int)ns, c->stream)))
        return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "RDS bits launch failed (%d)", rc);
    return 0;
}

inline char rds_char(unsigned b) { return b >= 0x20 && b <= 0x7E ? (char)b : ' '; }

inline unsigned word16(const uint8_t* b) {  // the 16 information bits of the 26-bit block at b
    unsigned v = 0;
    for (int k = 0; k < 16; k++) v = (v << 1) | (b[k] & 1u);
    return v;
}

void rds_group(fmrx_rds_info* io, unsigned a, unsigned b, unsigned cw, unsigned d) {
    io->groups++;
    io->pi = (uint16_t)a;
    io->tp = (uint8_t)((b >> 10) & 1);
    io->pty = (uint8_t)((b >> 5) & 0x1F);
    const unsigned type = b >> 12, version = (b >> 11) & 1;
    if (type == 0) {
        const unsigned at = 2 * (b & 3);
        io->ps[at] = rds_char(d >> 8);
        io->ps[at + 1] = rds_char(d & 0xFF);
    } else if (type == 2) {
        const uint8_t ab = (uint8_t)((b >> 4) & 1);
        if (ab != io->rt_ab) std::memset(io->rt, ' ', 64);
        io->rt_ab = ab;
        if (version == 0) {
            const unsigned at = 4 * (b & 15);
            io->rt[at] = rds_char(cw >> 8);
            io->rt[at + 1] = rds_char(cw & 0xFF);
            io->rt[at + 2] = rds_char(d >> 8);
            io->rt[at + 3] = rds_char(d & 0xFF);
        } else {
            const unsigned at = 2 * (b & 15);
            io->rt[at] = rds_char(d >> 8);
            io->rt[at + 1] = rds_char(d & 0xFF);
        }
    }
}

}  // namespace

namespace fmrx {

size_t rds_granule_blocks(const fmrx_ctx* c) {
    const size_t per_window = (size_t)(kRdsbWin / kRdsbUp) * (size_t)(c->geo.bp_fs / 2000);  // mixer samples a window
    const size_t g = std::lcm((size_t)c->geo.if_samples, per_window) / (size_t)c->geo.if_samples;
    return std::lcm(g, c->wide.ratio.blocks);
}

int check_rds_blocks(const fmrx_ctx* c, size_t n_blocks) {
    const size_t g = rds_granule_blocks(c);
    if (n_blocks % g != 0)
        return fail(FMRX_EINVAL, "%zu blocks: an RDS call takes whole granules of %zu blocks", n_blocks, g);
    return 0;
}

// the symbol-rate resampler's prototype: 101 taps a phase at 19 bp_fs, gain 19
int init_rds_bits(fmrx_ctx* c) {
    const size_t ns = c->cfg.n_streams;
    std::vector<float> taps(kRdsbTaps);
    design_lpf(taps.data(), (float)c->geo.bp_fs * (float)kRdsbUp, 3000.0f, kRdsbTaps, kRdsbUp);
    c->rdsb.info.resize(ns);
    c->rdss.ext.resize(ns);
    int rc = c->rdsb.hist.ensure((size_t)kRdsbHist * ns);
    if (!rc) rc = c->rdsb.state.ensure((size_t)kRdsbStateBytes * ns);
    return rc ? rc : upload(c->rdsb.taps, taps.data(), taps.size(), "RDS tap upload");
}

int reset_rds_bits(fmrx_ctx* c) {
    const size_t ns = c->cfg.n_streams;
    HIPCHK(hipMemsetAsync(c->rdsb.hist.p, 0, sizeof(float) * kRdsbHist * ns, c->stream));
    // zero symbols and bit count; the sign and the chip in front of the stream count as 1
    HIPCHK(hipMemsetAsync(c->rdsb.state.p, 0, (size_t)kRdsbStateBytes * ns, c->stream));
    HIPCHK(hipMemset2DAsync(c->rdsb.state.p, kRdsbStateBytes, 1, 2, ns, c->stream));
    for (auto& io : c->rdsb.info) fmrx_rds_info_init(&io);
    c->rdsb.pending = 0;
    reset_rds_sync(c);
    return 0;
}

int rds_decode_enqueue(fmrx_ctx* c, const float* d_demod, size_t demod_stride, size_t n_blocks) {
    const size_t ns = c->cfg.n_streams;
    const size_t n_if = n_blocks * c->geo.if_samples;
    const size_t n_sym = n_if * kRdsbUp / (size_t)(c->geo.bp_fs / 2000) / kRdsbWin * kRdsbSyms;
    c->rdsb.pending = 0;
    int rc;
    if ((rc = c->rdsb.mix.ensure(ns * n_if)) || (rc = c->rdsb.out.ensure(2 * ns * n_sym))) return rc;
    if ((rc = run_rds(c, d_demod, demod_stride, n_if, c->rdsb.mix.p, nullptr, nullptr))) return rc;
    if ((rc = run_rds_bits(c, c->rdsb.mix.p, n_if, n_blocks, c->rdsb.out.p, c->rdsb.out.p + ns * n_sym, nullptr,
                           nullptr)))
        return rc;
    c->rdsb.host.resize(2 * ns * n_sym);
    HIPCHK(hipMemcpyAsync(c->rdsb.host.data(), c->rdsb.out.p, 2 * ns * n_sym, hipMemcpyDeviceToHost, c->stream));
    c->rdsb.pending = n_sym;
    // the block sync over the same bits (fmrx_set_rds_sync), behind the copy
    if (c->rdss.on && (rc = rds_sync_enqueue(c, c->rdsb.out.p, n_sym))) return rc;
    return 0;
}

int rds_decode_finish(fmrx_ctx* c) {
    const size_t ns = c->cfg.n_streams, n = c->rdsb.pending;
    if (n == 0) return 0;
    c->rdsb.pending = 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t s = 0; s < ns; s++) {
        int rc = fmrx_rds_parse(&c->rdsb.info[s], c->rdsb.host.data() + s * n, c->rdsb.host.data() + (ns + s) * n, n);
        if (rc) return rc;
    }
    return rds_sync_finish(c);
}

}  // namespace fmrx

extern "C" {

int fmrx_rds_granule(const fmrx_ctx* c, size_t* blocks) {
    CtxLock lock_(c);
    if (!c || !blocks) return fail(FMRX_EINVAL, "null argument");
    *blocks = rds_granule_blocks(c);
    return FMRX_OK;
}

int fmrx_rds_bits_device(fmrx_ctx* c, const float* d_rds, size_t n_blocks, uint8_t* d_bits, uint8_t* d_codes,
                         uint8_t* d_win, float* d_y) {
    CtxLock lock_(c);
    if (!c || !d_rds) return fail(FMRX_EINVAL, "null argument");
    int rc = check_rds_blocks(c, n_blocks);
    if (rc || n_blocks == 0) return rc;
    if ((rc = set_device(c))) return rc;
    return run_rds_bits(c, d_rds, n_blocks * c->geo.if_samples, n_blocks, d_bits, d_codes, d_win, d_y);
}

int fmrx_rds_bits(fmrx_ctx* c, const float* rds, size_t n_blocks, uint8_t* bits, uint8_t* codes, uint8_t* win,
                  float* y) {
    CtxLock lock_(c);
    if (!c || !rds) return fail(FMRX_EINVAL, "null argument");
    int rc = check_rds_blocks(c, n_blocks);
    if (rc || n_blocks == 0) return rc;
    if ((rc = set_device(c))) return rc;
    const size_t ns = c->cfg.n_streams;
    const size_t n_if = n_blocks * c->geo.if_samples;
    const size_t n_out = n_if * kRdsbUp / (size_t)(c->geo.bp_fs / 2000), n_win = n_out / kRdsbWin, n_sym = n_win * kRdsbSyms;
    if ((rc = c->io.f32.ensure(ns * n_if)) || (rc = c->rdsb.out.ensure(ns * (2 * n_sym + 2 * n_win))) ||
        (y && (rc = c->io.scratch.ensure(ns * n_out))))
        return rc;
    uint8_t* d_bits = c->rdsb.out.p;
    uint8_t* d_codes = d_bits + ns * n_sym;
    uint8_t* d_win = d_codes + ns * n_sym;
    HIPCHK(hipMemcpyAsync(c->io.f32.p, rds, sizeof(float) * ns * n_if, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_rds_bits(c, c->io.f32.p, n_if, n_blocks, d_bits, d_codes, d_win, y ? c->io.scratch.p : nullptr))) return rc;
    if (bits) HIPCHK(hipMemcpyAsync(bits, d_bits, ns * n_sym, hipMemcpyDeviceToHost, c->stream));
    if (codes) HIPCHK(hipMemcpyAsync(codes, d_codes, ns * n_sym, hipMemcpyDeviceToHost, c->stream));
    if (win) HIPCHK(hipMemcpyAsync(win, d_win, ns * 2 * n_win, hipMemcpyDeviceToHost, c->stream));
    if (y) HIPCHK(hipMemcpyAsync(y, c->io.scratch.p, sizeof(float) * ns * n_out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FMRX_OK;
}

int fmrx_rds_info_init(fmrx_rds_info* io) {
    if (!io) return fail(FMRX_EINVAL, "null argument");
    std::memset(io, 0, sizeof *io);
    std::memset(io->ps, ' ', 8);
    std::memset(io->rt, ' ', 64);
    return FMRX_OK;
}

int fmrx_rds_parse(fmrx_rds_info* io, const uint8_t* bits, const uint8_t* codes, size_t n) {
    if (!io || ((!bits || !codes) && n)) return fail(FMRX_EINVAL, "null argument");
    if (io->tail_n > FMRX_RDS_TAIL) return fail(FMRX_EINVAL, "fmrx_rds_info: tail of %d bits", (int)io->tail_n);
    if (n == 0) return FMRX_OK;
    // the carried tail in front of the new bits: a group is judged at its last bit, 103 after its first
    const size_t t = io->tail_n, total = t + n;
    std::vector<uint8_t> b(total), cd(total);
    std::memcpy(b.data(), io->tail_bits, t);
    std::memcpy(cd.data(), io->tail_codes, t);
    std::memcpy(b.data() + t, bits, n);
    std::memcpy(cd.data() + t, codes, n);
    for (size_t j = t; j < total; j++) {
        io->bits++;
        if (cd[j]) io->blocks++;
        if (j < FMRX_RDS_TAIL || cd[j] != 5 || (cd[j - 26] != 3 && cd[j - 26] != 4) || cd[j - 52] != 2 || cd[j - 78] != 1)
            continue;
        const uint8_t* g = b.data() + (j - FMRX_RDS_TAIL);
        rds_group(io, word16(g), word16(g + 26), word16(g + 52), word16(g + 78));
    }
    const size_t keep = std::min<size_t>(total, FMRX_RDS_TAIL);
    std::memcpy(io->tail_bits, b.data() + (total - keep), keep);
    std::memcpy(io->tail_codes, cd.data() + (total - keep), keep);
    io->tail_n = (uint8_t)keep;
    return FMRX_OK;
}

int fmrx_rds_decode_device(fmrx_ctx* c, const float* d_demod, size_t n_blocks) {
    CtxLock lock_(c);
    if (!c || !d_demod) return fail(FMRX_EINVAL, "null argument");
    int rc = check_rds_blocks(c, n_blocks);
    if (rc || n_blocks == 0) return rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = rds_decode_enqueue(c, d_demod, n_blocks * c->geo.if_samples, n_blocks))) return rc;
    return rds_decode_finish(c);
}

int fmrx_rds_decode(fmrx_ctx* c, const float* demod, size_t n_blocks) {
    CtxLock lock_(c);
    if (!c || !demod) return fail(FMRX_EINVAL, "null argument");
    int rc = check_rds_blocks(c, n_blocks);
    if (rc || n_blocks == 0) return rc;
    if ((rc = set_device(c))) return rc;
    const size_t n = (size_t)c->cfg.n_streams * n_blocks * c->geo.if_samples;
    if ((rc = c->io.f32.ensure(n))) return rc;
    HIPCHK(hipMemcpyAsync(c->io.f32.p, demod, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    if ((rc = rds_decode_enqueue(c, c->io.f32.p, n_blocks * c->geo.if_samples, n_blocks))) return rc;
    return rds_decode_finish(c);
}

int fmrx_rds_info_get(const fmrx_ctx* c, int stream, fmrx_rds_info* out) {
    CtxLock lock_(c);
    if (!c || !out) return fail(FMRX_EINVAL, "null argument");
    if (stream < 0 || stream >= c->cfg.n_streams) return fail(FMRX_EINVAL, "stream %d of %d", stream, c->cfg.n_streams);
    *out = c->rdsb.info[(size_t)stream];
    return FMRX_OK;
}

int fmrx_set_rds(fmrx_ctx* c, int on) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null argument");
    c->rdsb.on = on != 0;
    return FMRX_OK;
}

}  // extern "C"
