// rds_sync.hip — RDS block sync: the bits of rds_bits.hip to accepted 26-bit blocks.
// Per stream, over a call's domain (the carried bits followed by the new ones):
//
//   s[i]        = syndrome of the 26 bits ending at i                      as rdsb_code_kernel
//   exact[i]    = the slots u (A, B, C*, D) whose offset word s[i] equals
//   cand[u][i]  = the slot's information word where s[i] ^ offset is 0 or a burst the table corrects
//   votes[u][i] = #{j in -J..J, j != 0 : exact[i + 26 j] has slot (u + j) mod 4}
//   rec[i]      = the slot with a candidate and the most votes >= V (lowest u on a tie)
//
// and the accepted records of each stream packed in bit order.  Signs and integers only; nothing is
// serial in time: one lane a bit (a position), one workgroup a stream for the packing and the carry.
#include <hip/hip_runtime.h>

#include "fmrx_internal.h"

namespace fmrx {

namespace {

constexpr unsigned kNoBurst = 0xFFFFFFFFu;
constexpr unsigned kOffA = 0x0FCu, kOffB = 0x198u, kOffC = 0x168u, kOffCp = 0x350u, kOffD = 0x1B4u;
constexpr unsigned kValid = 1u << 16, kCorrected = 1u << 17, kCPrime = 1u << 18;

// fmrx_rds_block_rec (include/fmrx.h), as the packing kernel stores it
struct Block {
    unsigned long long bit;
    uint16_t info;
    uint8_t slot, c_prime, corrected, votes;
    uint8_t pad[2];
};
static_assert(sizeof(Block) == 16, "fmrx_rds_block_rec is 16 bytes");

__device__ inline unsigned dom_bit(const RdsSyncLaunch& L, int s, int d) {  // 0 <= d < n_dom
    return (d < L.n_carry ? L.carry[(size_t)s * kRdsSyncCarry + (kRdsSyncCarry - L.n_carry + d)]
                          : L.bits[(size_t)s * L.bits_stride + (size_t)(d - L.n_carry)]) & 1u;
}

// the slot's candidate for syndrome difference e (and e2 of the second offset word, C'): exact first
__device__ inline unsigned slot_cand(const unsigned* tab, unsigned word, unsigned e, unsigned e2, bool two) {
    if (e == 0) return (word >> 10) | kValid;
    if (two && e2 == 0) return (word >> 10) | kValid | kCPrime;
    const unsigned p = tab[e];
    if (p != kNoBurst) return ((word ^ p) >> 10) | kValid | kCorrected;
    if (two) {
        const unsigned p2 = tab[e2];
        if (p2 != kNoBurst) return ((word ^ p2) >> 10) | kValid | kCorrected | kCPrime;
    }
    return 0;
}

// One lane a bit of the domain: the word, its syndrome, the exact mask and the four candidates.
__global__ void __launch_bounds__(256) rdss_cand_kernel(RdsSyncLaunch L) {
    __shared__ unsigned tab[kRdsSyncTable];
    for (int k = threadIdx.x; k < kRdsSyncTable; k += 256) tab[k] = L.table[k];
    __syncthreads();
    const int d = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (d >= L.n_dom) return;
    unsigned mask = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (d >= 25) {  // a whole word inside the domain (positions below are never read: the carry reaches 25 further back)
        unsigned word = 0, reg = 0;
        for (int k = d - 25; k <= d; k++) {
            const unsigned bit = dom_bit(L, s, k);
            word = (word << 1) | bit;
            reg = (reg << 1) | bit;
            if (reg & 0x400u) reg ^= 0x5B9u;
        }
        mask = (reg == kOffA ? 1u : 0u) | (reg == kOffB ? 2u : 0u) | ((reg == kOffC || reg == kOffCp) ? 4u : 0u) |
               (reg == kOffD ? 8u : 0u);
        c0 = slot_cand(tab, word, reg ^ kOffA, 0, false);
        c1 = slot_cand(tab, word, reg ^ kOffB, 0, false);
        c2 = slot_cand(tab, word, reg ^ kOffC, reg ^ kOffCp, true);
        c3 = slot_cand(tab, word, reg ^ kOffD, 0, false);
    }
    L.exact[(size_t)s * L.n_dom + d] = (uint8_t)mask;
    uint32_t* cand = L.cand + (size_t)s * 4 * L.n_dom + d;
    cand[0] = c0;
    cand[(size_t)L.n_dom] = c1;
    cand[2 * (size_t)L.n_dom] = c2;
    cand[3 * (size_t)L.n_dom] = c3;
}

// One lane a judged position: 2 J loads of the exact mask at stride 26, the four counts, the slot.
__global__ void __launch_bounds__(256) rdss_vote_kernel(RdsSyncLaunch L) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (t >= L.n_judge) return;
    const int d = L.j0 + t;  // < n_dom
    const uint8_t* ex = L.exact + (size_t)s * L.n_dom;
    unsigned v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 1; j <= kRdsSyncMaxJ; j++) {
        if (j > L.J) break;
        const int lo = d - 26 * j, hi = d + 26 * j;
        const unsigned ml = lo >= 0 ? ex[lo] : 0u;       // in front of the domain: no match
        const unsigned mh = hi < L.n_dom ? ex[hi] : 0u;  // not arrived (a flush): no match
#pragma unroll
        for (int u = 0; u < 4; u++) {
            v[u] += (ml >> ((u - j) & 3)) & 1u;
            v[u] += (mh >> ((u + j) & 3)) & 1u;
        }
    }
    const uint32_t* cand = L.cand + (size_t)s * 4 * L.n_dom + d;
    unsigned rec = 0, best = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const unsigned c = cand[(size_t)u * L.n_dom];
        if ((c & kValid) && v[u] >= (unsigned)L.V && v[u] > best) {  // V >= 1, so best = 0 means none yet
            best = v[u];
            rec = c | ((unsigned)u << 19) | (v[u] << 21) | (1u << 31);
        }
    }
    L.rec[(size_t)s * L.n_judge + t] = rec;
}

// One workgroup a stream walks its judged positions in chunks of 256: a ballot a wave and the waves'
// totals in LDS give each accepted record its place in the stream's list.
__global__ void __launch_bounds__(256) rdss_pack_kernel(RdsSyncLaunch L) {
    __shared__ unsigned wave_n[4];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t* rec = L.rec + (size_t)s * L.n_judge;
    Block* out = (Block*)L.blocks + (size_t)s * L.max_blocks;
    unsigned total = 0;
    for (int base = 0; base < L.n_judge; base += 256) {
        const int t = base + tid;
        const unsigned r = t < L.n_judge ? rec[t] : 0u;
        const bool take = (r >> 31) != 0;
        const unsigned long long m = __ballot(take);
        if (lane == 0) wave_n[wave] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned at = total + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) at += wave_n[w];
        const unsigned chunk = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        if (take && at < L.max_blocks) {
            Block b;
            b.bit = L.base + (unsigned long long)(L.j0 + t);
            b.info = (uint16_t)(r & 0xFFFFu);
            b.slot = (uint8_t)((r >> 19) & 3u);
            b.c_prime = (uint8_t)((r >> 18) & 1u);
            b.corrected = (uint8_t)((r >> 17) & 1u);
            b.votes = (uint8_t)((r >> 21) & 31u);
            b.pad[0] = b.pad[1] = 0;
            out[at] = b;
        }
        total += chunk;
        __syncthreads();  // wave_n is rewritten by the next chunk
    }
    if (tid == 0) L.counts[s] = total;
}

// The carry for the next call, one workgroup a stream, after everything that reads the old one: the
// last n_keep bits of the domain, right-aligned.  Every lane reads before any lane writes.
__global__ void __launch_bounds__(512) rdss_carry_kernel(RdsSyncLaunch L) {
    const int s = blockIdx.x, t = threadIdx.x;
    unsigned bit = 0;
    if (t < L.n_keep) bit = dom_bit(L, s, L.n_dom - L.n_keep + t);
    __syncthreads();
    if (t < L.n_keep) L.carry[(size_t)s * kRdsSyncCarry + (kRdsSyncCarry - L.n_keep + t)] = (uint8_t)bit;
}

}  // namespace

int launch_rds_sync(const RdsSyncLaunch& L, int n_streams, hipStream_t s) {
    if (n_streams <= 0) return 0;
    if (L.n_carry < 0 || L.n_carry > kRdsSyncCarry || L.n_new < 0 || L.n_dom != L.n_carry + L.n_new || L.J < 1 ||
        L.J > kRdsSyncMaxJ || L.V < 1 || L.j0 < 0 || L.n_judge < 0 || L.j0 + L.n_judge > L.n_dom || L.n_keep < 0 ||
        L.n_keep > kRdsSyncCarry || L.n_keep > L.n_dom)
        return -1;
    if (L.n_judge > 0) {
        hipLaunchKernelGGL(rdss_cand_kernel, dim3((L.n_dom + 255) / 256, n_streams), dim3(256), 0, s, L);
        hipLaunchKernelGGL(rdss_vote_kernel, dim3((L.n_judge + 255) / 256, n_streams), dim3(256), 0, s, L);
    }
    hipLaunchKernelGGL(rdss_pack_kernel, dim3(n_streams), dim3(256), 0, s, L);  // n_judge = 0: the counts alone
    if (L.n_new > 0) hipLaunchKernelGGL(rdss_carry_kernel, dim3(n_streams), dim3(512), 0, s, L);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace fmrx
