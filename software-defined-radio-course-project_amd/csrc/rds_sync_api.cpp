// rds_sync_api.cpp — the RDS block sync's entry points: the burst table, the accepted
// blocks of bit rows (rds_sync.hip), the host block-wise group parser, and the hooks that run both
// behind the RDS decode into the context's per-stream extended info.
#include <cstring>

#include "ctx.h"

using namespace fmrx;

namespace {

constexpr int kMaxBurst = 5;

inline unsigned syndrome26(unsigned word) {  // the remainder of the 26-bit word by the generator
    unsigned reg = 0;
    for (int k = 25; k >= 0; k--) {
        reg = (reg << 1) | ((word >> k) & 1u);
        if (reg & 0x400u) reg ^= 0x5B9u;
    }
    return reg;
}

// table (may be null) and the patterns placed; false: two bursts share a syndrome
bool sync_design(int B, uint32_t* table, int* patterns) {
    uint32_t tab[kRdsSyncTable];
    for (auto& e : tab) e = FMRX_RDS_NO_BURST;
    tab[0] = 0;
    int n = 0;
    for (int len = 1; len <= B; len++) {
        const unsigned inner = len <= 2 ? 1u : 1u << (len - 2);
        for (unsigned mid = 0; mid < inner; mid++) {
            const unsigned pat = len == 1 ? 1u : (1u << (len - 1)) | (mid << 1) | 1u;
            for (int shift = 0; shift + len <= 26; shift++) {
                const unsigned s = syndrome26(pat << shift);
                if (tab[s] != FMRX_RDS_NO_BURST) return false;
                tab[s] = pat << shift;
                n++;
            }
        }
    }
    if (table) std::memcpy(table, tab, sizeof tab);
    if (patterns) *patterns = n;
    return true;
}

int check_sync_config(const fmrx_rds_sync_config* cfg) {
    if (cfg->J < 1 || cfg->J > kRdsSyncMaxJ || cfg->V < 1 || cfg->V > 2 * cfg->J || cfg->B < 0 || cfg->B > kMaxBurst)
        return fail(FMRX_EINVAL, "RDS sync config J = %d, V = %d, B = %d: 1 <= J <= %d, 1 <= V <= 2 J, 0 <= B <= %d", cfg->J,
                    cfg->V, cfg->B, kRdsSyncMaxJ, kMaxBurst);
    return 0;
}

// the table of cfg's B on the device and the carry rows, and cfg taken as the stream's
int sync_prepare(fmrx_ctx* c, const fmrx_rds_sync_config* cfg) {
    fmrx_rds_sync_config def;
    (void)fmrx_rds_sync_config_default(&def);
    if (!cfg) cfg = &def;
    int rc = check_sync_config(cfg);
    if (rc) return rc;
    const auto& cur = c->rdss.cfg;
    if (c->rdss.seen && (cur.J != cfg->J || cur.V != cfg->V || cur.B != cfg->B))
        return fail(FMRX_EINVAL, "RDS sync config changed inside a stream (J %d V %d B %d, now %d %d %d): fmrx_reset first", cur.J,
                    cur.V, cur.B, cfg->J, cfg->V, cfg->B);
    if ((rc = c->rdss.table.ensure(kRdsSyncTable)) || (rc = c->rdss.carry.ensure((size_t)kRdsSyncCarry * c->cfg.n_streams)))
        return rc;
    if (c->rdss.table_b != cfg->B) {
        uint32_t tab[kRdsSyncTable];
        if (!sync_design(cfg->B, tab, nullptr)) return fail(FMRX_ESTATE, "RDS sync: two bursts of length <= %d share a syndrome", cfg->B);
        HIPCHK(hipMemcpyAsync(c->rdss.table.p, tab, sizeof tab, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));  // tab is on this call's stack
        c->rdss.table_b = cfg->B;
    }
    c->rdss.cfg = *cfg;
    return 0;
}

// The stage over n_new more bits a stream at d_bits (flush: and every pending position), enqueued:
// the records to d_blocks (rows of max_blocks), the counts to d_counts.
int run_rds_sync(fmrx_ctx* c, const uint8_t* d_bits, size_t bits_stride, size_t n_new, bool flush, fmrx_rds_block_rec* d_blocks,
                 size_t max_blocks, uint32_t* d_counts) {
    const size_t ns = c->cfg.n_streams;
    const int J = c->rdss.cfg.J;
    const uint64_t keep = 25 + 52 * (uint64_t)J, ahead = 26 * (uint64_t)J;
    if (n_new > ((size_t)1 << 30)) return fail(FMRX_EINVAL, "%zu bits: too many for one RDS sync call", n_new);
    const uint64_t seen = c->rdss.seen, total = seen + n_new;
    const uint64_t n_carry = std::min(seen, keep), base = seen - n_carry;
    const uint64_t upto = flush ? total : (total > ahead ? total - ahead : 0);  // positions below it are judged after this call
    const uint64_t from = c->rdss.judged, to = std::max(from, upto);
    RdsSyncLaunch L{};
    L.bits = d_bits;
    L.bits_stride = bits_stride;
    L.carry = c->rdss.carry.p;
    L.table = c->rdss.table.p;
    L.base = base;
    L.n_carry = (int)n_carry;
    L.n_new = (int)n_new;
    L.n_dom = L.n_carry + L.n_new;
    L.j0 = (int)(from - base);  // from >= base: a call leaves at most `ahead` positions pending, the carry holds more
    L.n_judge = (int)(to - from);
    L.n_keep = (int)std::min<uint64_t>(total, keep);
    L.J = J;
    L.V = c->rdss.cfg.V;
    L.max_blocks = (unsigned)std::min<size_t>(max_blocks, 0xFFFFFFFFu);
    int rc = c->rdss.work.ensure(ns * (5 * (size_t)L.n_dom + (size_t)L.n_judge) + 1);
    if (rc) return rc;
    L.cand = c->rdss.work.p;
    L.rec = L.cand + ns * 4 * (size_t)L.n_dom;
    L.exact = reinterpret_cast<uint8_t*>(L.rec + ns * (size_t)L.n_judge);  // ns x n_dom bytes in ns x n_dom words
    L.blocks = d_blocks;
    L.counts = d_counts;
    if ((rc = launch_rds_sync(L, (int)ns, c->stream)))
        return fail(rc == -1 ? FMRX_EINVAL : FMRX_EHIP, "RDS sync launch failed (%d)", rc);
    c->rdss.seen = total;
    c->rdss.judged = to;
    return 0;
}

// positions a call of n_new bits (or a flush) judges: the rows a caller's record list needs at most
size_t sync_judged(const fmrx_ctx* c, size_t n_new, bool flush) {
    const uint64_t ahead = 26 * (uint64_t)c->rdss.cfg.J, total = c->rdss.seen + n_new;
    const uint64_t upto = flush ? total : (total > ahead ? total - ahead : 0);
    return upto > c->rdss.judged ? (size_t)(upto - c->rdss.judged) : 0;
}

// the host forms' tail: counts, then each stream's first min(count, cap) records (one 2-D copy)
int fetch_blocks(fmrx_ctx* c, size_t cap, fmrx_rds_block_rec* blocks, size_t max_blocks, uint32_t* counts) {
    const size_t ns = c->cfg.n_streams;
    c->rdss.counts_host.resize(ns);
    HIPCHK(hipMemcpyAsync(c->rdss.counts_host.data(), c->rdss.counts.p, sizeof(uint32_t) * ns, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    size_t most = 0;
    for (size_t s = 0; s < ns; s++) most = std::max<size_t>(most, std::min<size_t>(c->rdss.counts_host[s], cap));
    c->rdss.host.resize(ns * most);
    if (most)
        HIPCHK(hipMemcpy2D(c->rdss.host.data(), most * sizeof(fmrx_rds_block_rec), c->rdss.blocks.p, cap * sizeof(fmrx_rds_block_rec),
                           most * sizeof(fmrx_rds_block_rec), ns, hipMemcpyDeviceToHost));
    c->rdss.most = most;
    for (size_t s = 0; s < ns; s++) {
        if (counts) counts[s] = c->rdss.counts_host[s];
        if (blocks && max_blocks)
            std::memcpy(blocks + s * max_blocks, c->rdss.host.data() + s * most,
                        sizeof(fmrx_rds_block_rec) * std::min<size_t>({(size_t)c->rdss.counts_host[s], cap, max_blocks}));
    }
    return 0;
}

int parse_fetched(fmrx_ctx* c, size_t cap, uint64_t n_bits, int flush) {
    for (size_t s = 0; s < (size_t)c->cfg.n_streams; s++) {
        int rc = fmrx_rds_parse_blocks(&c->rdss.ext[s], c->rdss.host.data() + s * c->rdss.most,
                                       std::min<size_t>(c->rdss.counts_host[s], cap), n_bits, flush);
        if (rc) return rc;
    }
    return 0;
}

inline char rds_char(unsigned b) { return b >= 0x20 && b <= 0x7E ? (char)b : ' '; }

const fmrx_rds_block_rec* tail_find(const fmrx_rds_ext* x, uint64_t bit, int slot) {
    for (int k = 0; k < x->tail_n; k++)
        if (x->tail[k].bit == bit && x->tail[k].slot == slot) return &x->tail[k];
    return nullptr;
}

// year, month and day of an MJD by IEC 62106 annex G in integers (good from 1900-03-01 to 2100-02-28; zeros below
// 15079, where Y' would be negative)
void mjd_date(uint32_t mjd, uint16_t* year, uint8_t* month, uint8_t* day) {
    *year = 0, *month = 0, *day = 0;
    if (mjd < 15079) return;
    const int64_t m0 = mjd;
    const int64_t y = (m0 * 100 - 1507820) / 36525, yd = (y * 1461) / 4;
    const int64_t m = ((m0 - yd) * 10000 - 149561000) / 306001;
    const int64_t d = m0 - 14956 - yd - (m * 306001) / 10000;
    const int64_t k = (m == 14 || m == 15) ? 1 : 0;
    *year = (uint16_t)(1900 + y + k);
    *month = (uint8_t)(m - 1 - 12 * k);
    *day = (uint8_t)d;
}

// close the B block r with whatever of A, C*, D the tail holds
void ext_group(fmrx_rds_ext* x, const fmrx_rds_block_rec& r) {
    const fmrx_rds_block_rec* a = r.bit >= 26 ? tail_find(x, r.bit - 26, 0) : nullptr;
    const fmrx_rds_block_rec* c = tail_find(x, r.bit + 26, 2);
    const fmrx_rds_block_rec* d = tail_find(x, r.bit + 52, 3);
    if (a && a->corrected && !(x->pi_set && a->info == x->pi)) a = nullptr;
    if (a && c && d) x->groups++;
    else x->partial_groups++;
    const unsigned b = r.info, type = b >> 12, version = (b >> 11) & 1;
    x->tp = (uint8_t)((b >> 10) & 1);
    x->pty = (uint8_t)((b >> 5) & 0x1F);
    const bool c_plain = c && !c->c_prime;
    const unsigned cw = c ? c->info : 0, dw = d ? d->info : 0;
    const bool b_sure = !r.corrected, c_sure = b_sure && c && !c->corrected, d_sure = b_sure && d && !d->corrected;
    // two characters: a block pair without a correction always writes and marks the places its own (sure);
    // one with a correction writes only places not so marked
    auto put2 = [](char* text, auto* marks, unsigned at, unsigned w, bool sure) {
        const char ch[2] = {rds_char(w >> 8), rds_char(w & 0xFF)};
        for (unsigned k = 0; k < 2; k++) {
            const uint64_t m = 1ull << (at + k);
            if (sure) {
                text[at + k] = ch[k];
                *marks |= (decltype(*marks + 0))m;
            } else if (!(*marks & m)) {
                text[at + k] = ch[k];
            }
        }
    };
    // the A/B flag rule: a change clears the text; a corrected B block may not change it (false: skip the group's text)
    auto flag = [&](char* text, size_t len, auto* marks, uint8_t* cur, uint8_t ab) {
        if (ab == *cur) return true;
        if (!b_sure) return false;
        std::memset(text, ' ', len);
        *marks = 0;
        *cur = ab;
        return true;
    };
    if (type == 0) {
        const unsigned seg = b & 3;
        x->ta = (uint8_t)((b >> 4) & 1);
        x->ms = (uint8_t)((b >> 3) & 1);
        x->di = (uint8_t)((x->di & ~(1u << (3 - seg))) | (((b >> 2) & 1) << (3 - seg)));
        if (d) put2(x->ps, &x->ps_sure, 2 * seg, dw, d_sure);
        if (version == 0 && c_plain && c_sure) {
            const unsigned codes[2] = {cw >> 8, cw & 0xFF};
            for (unsigned code : codes) {
                if (code >= 1 && code <= 204) {
                    bool have = false;
                    for (int k = 0; k < x->af_n; k++) have = have || x->af[k] == code;
                    if (!have && x->af_n < FMRX_RDS_MAX_AF) x->af[x->af_n++] = (uint8_t)code;
                } else if (code >= 224 && code <= 249) {
                    x->af_count = (uint8_t)(code - 224);
                }
            }
        }
    } else if (type == 2) {
        if (flag(x->rt, 64, &x->rt_sure, &x->rt_ab, (uint8_t)((b >> 4) & 1))) {
            if (version == 0) {
                const unsigned at = 4 * (b & 15);
                if (c_plain) put2(x->rt, &x->rt_sure, at, cw, c_sure);
                if (d) put2(x->rt, &x->rt_sure, at + 2, dw, d_sure);
            } else if (d) {
                put2(x->rt, &x->rt_sure, 2 * (b & 15), dw, d_sure);
            }
        }
    } else if (type == 4 && version == 0 && c_plain && c_sure && d_sure) {
        const unsigned hour = ((cw & 1) << 4) | (dw >> 12), minute = (dw >> 6) & 0x3F;
        if (hour < 24 && minute < 60) {
            x->ct_set = 1;
            x->ct_mjd = ((b & 3) << 15) | (cw >> 1);
            x->ct_hour = (uint8_t)hour;
            x->ct_minute = (uint8_t)minute;
            x->ct_offset = (int8_t)(((dw >> 5) & 1) ? -(int)(dw & 0x1F) : (int)(dw & 0x1F));
            mjd_date(x->ct_mjd, &x->ct_year, &x->ct_month, &x->ct_day);
        }
    } else if (type == 10 && version == 0) {
        if (flag(x->ptyn, 8, &x->ptyn_sure, &x->ptyn_ab, (uint8_t)((b >> 4) & 1))) {
            const unsigned at = 4 * (b & 1);
            if (c_plain) put2(x->ptyn, &x->ptyn_sure, at, cw, c_sure);
            if (d) put2(x->ptyn, &x->ptyn_sure, at + 2, dw, d_sure);
        }
    }
}

// close the open B blocks whose D position lies before `before` (all of them when `all`)
void ext_close(fmrx_rds_ext* x, uint64_t before, bool all) {
    for (int k = 0; k < x->tail_n; k++)
        if (x->tail[k].slot == 1 && !x->tail_done[k] && (all || x->tail[k].bit + 52 < before)) {
            x->tail_done[k] = 1;
            ext_group(x, x->tail[k]);
        }
}

}  // namespace

namespace fmrx {

void reset_rds_sync(fmrx_ctx* c) {
    c->rdss.seen = 0;
    c->rdss.judged = 0;
    c->rdss.pending = false;
    for (auto& x : c->rdss.ext) fmrx_rds_ext_init(&x);
}

int rds_sync_enqueue(fmrx_ctx* c, const uint8_t* d_bits, size_t n_bits) {
    const size_t ns = c->cfg.n_streams;
    c->rdss.pending = false;
    int rc = sync_prepare(c, nullptr);
    if (rc) return rc;
    const size_t cap = sync_judged(c, n_bits, false);
    if ((rc = c->rdss.blocks.ensure(ns * cap)) || (rc = c->rdss.counts.ensure(ns))) return rc;
    if ((rc = run_rds_sync(c, d_bits, n_bits, n_bits, false, c->rdss.blocks.p, cap, c->rdss.counts.p))) return rc;
    c->rdss.pending = true;
    c->rdss.cap = cap;
    c->rdss.bits = n_bits;
    return 0;
}

int rds_sync_finish(fmrx_ctx* c) {
    if (!c->rdss.pending) return 0;
    c->rdss.pending = false;
    int rc = fetch_blocks(c, c->rdss.cap, nullptr, 0, nullptr);
    return rc ? rc : parse_fetched(c, c->rdss.cap, c->rdss.bits, 0);
}

}  // namespace fmrx

extern "C" {

int fmrx_rds_sync_config_default(fmrx_rds_sync_config* cfg) {
    if (!cfg) return fail(FMRX_EINVAL, "null argument");
    cfg->J = 8;
    cfg->V = 3;
    cfg->B = 2;
    return FMRX_OK;
}

int fmrx_rds_sync_design(int B, uint32_t* table, int* patterns) {
    if (B < 0 || B > kMaxBurst) return fail(FMRX_EINVAL, "RDS sync: burst length %d outside 0 .. %d", B, kMaxBurst);
    if (!sync_design(B, table, patterns)) return fail(FMRX_ESTATE, "RDS sync: two bursts of length <= %d share a syndrome", B);
    return FMRX_OK;
}

int fmrx_rds_blocks_device(fmrx_ctx* c, const fmrx_rds_sync_config* cfg, const uint8_t* d_bits, size_t n_bits,
                           fmrx_rds_block_rec* d_blocks, size_t max_blocks, uint32_t* d_counts) {
    CtxLock lock_(c);
    if (!c || !d_counts || (!d_bits && n_bits) || (!d_blocks && max_blocks)) return fail(FMRX_EINVAL, "null argument");
    int rc = set_device(c);
    if (rc || (rc = sync_prepare(c, cfg))) return rc;
    return run_rds_sync(c, d_bits, n_bits, n_bits, false, d_blocks, max_blocks, d_counts);
}

int fmrx_rds_blocks(fmrx_ctx* c, const fmrx_rds_sync_config* cfg, const uint8_t* bits, size_t n_bits, fmrx_rds_block_rec* blocks,
                    size_t max_blocks, uint32_t* counts) {
    CtxLock lock_(c);
    if (!c || !counts || (!bits && n_bits) || (!blocks && max_blocks)) return fail(FMRX_EINVAL, "null argument");
    int rc = set_device(c);
    if (rc || (rc = sync_prepare(c, cfg))) return rc;
    const size_t ns = c->cfg.n_streams;
    if (n_bits > ((size_t)1 << 30)) return fail(FMRX_EINVAL, "%zu bits: too many for one RDS sync call", n_bits);
    const size_t cap = sync_judged(c, n_bits, false);
    if ((rc = c->rdss.in.ensure(ns * n_bits)) || (rc = c->rdss.blocks.ensure(ns * cap)) || (rc = c->rdss.counts.ensure(ns)))
        return rc;
    if (n_bits) HIPCHK(hipMemcpyAsync(c->rdss.in.p, bits, ns * n_bits, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_rds_sync(c, c->rdss.in.p, n_bits, n_bits, false, c->rdss.blocks.p, cap, c->rdss.counts.p))) return rc;
    return fetch_blocks(c, cap, blocks, max_blocks, counts);
}

int fmrx_rds_blocks_flush(fmrx_ctx* c, fmrx_rds_block_rec* blocks, size_t max_blocks, uint32_t* counts) {
    CtxLock lock_(c);
    if (!c || (!blocks && max_blocks)) return fail(FMRX_EINVAL, "null argument");
    if (c->rdss.seen == 0) {  // nothing given since the reset: nothing pending (and perhaps nothing allocated)
        if (counts) std::memset(counts, 0, sizeof(uint32_t) * (size_t)c->cfg.n_streams);
        return FMRX_OK;
    }
    int rc = set_device(c);
    if (rc) return rc;
    const size_t ns = c->cfg.n_streams, cap = sync_judged(c, 0, true);
    if ((rc = c->rdss.blocks.ensure(ns * cap)) || (rc = c->rdss.counts.ensure(ns))) return rc;
    if ((rc = run_rds_sync(c, nullptr, 0, 0, true, c->rdss.blocks.p, cap, c->rdss.counts.p))) return rc;
    if ((rc = fetch_blocks(c, cap, blocks, max_blocks, counts))) return rc;
    return c->rdss.on ? parse_fetched(c, cap, 0, 1) : FMRX_OK;
}

int fmrx_rds_ext_init(fmrx_rds_ext* io) {
    if (!io) return fail(FMRX_EINVAL, "null argument");
    std::memset(io, 0, sizeof *io);
    std::memset(io->ps, ' ', 8);
    std::memset(io->rt, ' ', 64);
    std::memset(io->ptyn, ' ', 8);
    return FMRX_OK;
}

int fmrx_rds_parse_blocks(fmrx_rds_ext* x, const fmrx_rds_block_rec* blocks, size_t n, uint64_t n_bits, int flush) {
    if (!x || (!blocks && n)) return fail(FMRX_EINVAL, "null argument");
    if (x->tail_n > FMRX_RDS_EXT_TAIL) return fail(FMRX_EINVAL, "fmrx_rds_ext: tail of %d records", (int)x->tail_n);
    for (size_t k = 0; k < n; k++)
        if (blocks[k].slot > 3) return fail(FMRX_EINVAL, "record %zu: slot %d", k, (int)blocks[k].slot);
    x->bits += n_bits;
    for (size_t k = 0; k < n; k++) {
        const fmrx_rds_block_rec& r = blocks[k];
        ext_close(x, r.bit, false);
        if (x->tail_n == FMRX_RDS_EXT_TAIL) {  // the oldest record leaves (an open B block with it)
            std::memmove(x->tail, x->tail + 1, sizeof(fmrx_rds_block_rec) * (FMRX_RDS_EXT_TAIL - 1));
            std::memmove(x->tail_done, x->tail_done + 1, FMRX_RDS_EXT_TAIL - 1);
            x->tail_n--;
        }
        x->tail[x->tail_n] = r;
        x->tail_done[x->tail_n++] = 0;
        if (r.corrected) x->corrected_blocks++;
        else x->exact_blocks++;
        if (r.slot == 0 && !r.corrected) {
            x->pi = r.info;
            x->pi_set = 1;
        }
        ext_close(x, r.bit + 1, false);
    }
    if (flush) ext_close(x, 0, true);
    return FMRX_OK;
}

int fmrx_set_rds_sync(fmrx_ctx* c, int on) {
    CtxLock lock_(c);
    if (!c) return fail(FMRX_EINVAL, "null argument");
    if (on) {  // the table and the carry now, so that a call allocates nothing but its work rows
        int rc = set_device(c);
        if (rc || (rc = sync_prepare(c, nullptr))) return rc;
    }
    c->rdss.on = on != 0;
    return FMRX_OK;
}

int fmrx_rds_ext_get(const fmrx_ctx* c, int stream, fmrx_rds_ext* out) {
    CtxLock lock_(c);
    if (!c || !out) return fail(FMRX_EINVAL, "null argument");
    if (stream < 0 || stream >= c->cfg.n_streams) return fail(FMRX_EINVAL, "stream %d of %d", stream, c->cfg.n_streams);
    *out = c->rdss.ext[(size_t)stream];
    return FMRX_OK;
}

}  // extern "C"
