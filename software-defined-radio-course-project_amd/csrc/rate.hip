// rate.hip — the rational down-converter in front of the tuner: a capture at cap_fs = rf_fs M / L
// (L / M in lowest terms, 2 <= L <= 48, L < M <= 125, M <= 10 L) -> per station: coarse rotation at
// the capture rate -> low-pass at the virtual rate M rf_fs -> interpolate by L, decimate by M -> cf32
// rows at rf_fs, which tuner.hip then reads as an FMRX_IQ_F32 stream tuned to the fine part of the
// offset.  Every station reads the ONE capture.  L and M are runtime values.
//
// Arithmetic (the contract the tests check bit for bit).  The split and the rotation
// are wide.hip's with N = 4 M / gcd(|q| L, 4 M), k = (q L / gcd) mod N.  With h the 16 M + 1 tap
// low-pass (cut-off 3 rf_fs / 8 at M rf_fs, gain L)
//   y[m] = sum h[k] x'[(m M - k) / L] over the k in 0..16 M with k = m M (mod L), ascending,
//   acc = fl(acc + fl(h[k] x)) from 0; pairs in front of the stream are 0.
//
// Decomposition.  A workgroup (four waves) walks a run of chunks of one station; a chunk is 64 L outputs
// = 64 M wide pairs, staged by all 256 threads into rows the waves share; the waves split the chunk's
// phases.  Lane t of a wave owns the outputs m = base + phi + L t for every phase phi < L: all lanes of
// a phase share k_0 = (phi M) mod L, hence the tap sequence h[k_0 + L i] (wave-uniform loads from the
// taps regrouped by phase), and lane t reads buffer pair t M + floor(phi M / L) - i behind the history.
// The rotated pairs sit in LDS in M polyphase rows, pair b of the buffer (HC M history pairs, HC =
// ceil(16 / L), then the chunk's) at [b mod M][b div M], so consecutive lanes read consecutive
// addresses for every tap.  Up to kR phases run side by side in a wave (one sequential sum each).  The outputs of a
// chunk go through LDS (rows of L | 1 pairs a lane) so that the global stores are coalesced.  The last
// HC columns of a chunk are the next chunk's history; the first chunk of a workgroup rebuilds its
// history from the raw pairs in front of it, and a phase of the rotator is a function of the absolute
// index alone, so there is no carried state.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dsp_device.h"
#include "iq_fmt.h"
#include "tuner.h"
#include "wide.h"

namespace fmrx {

namespace {

constexpr int kNT = kRateChunkLanes;  // lanes that share a phase: one wave
constexpr int kNW = 4;                // waves a workgroup: they share the chunk's rows and split its phases
constexpr int kNS = kNT * kNW;        // threads a workgroup
constexpr int kR = 4;                 // phases side by side
constexpr int kK = 4;                 // unit loads a lane in flight

// R phases phi0 .. phi0 + R - 1 of the chunk in xb, each one sequential sum over its taps in ascending
// k, the results to the hand-off rows.  The taps and where they read are wave-uniform loads.
template <int R>
__device__ inline void rate_phases(const float2* xb, float2* ob, const RateTap* __restrict__ hp, int phi0, int L, int M,
                                   int TS, int nmin, int rem, int tid) {
    float2v acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = float2v{0.0f, 0.0f};
    const RateTap* __restrict__ hrow = hp + phi0 * TS;
    const char* xt = reinterpret_cast<const char*>(xb + tid);
#pragma unroll 4
    for (int i = 0; i < nmin; i++) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const RateTap tp = hrow[r * TS + i];
            const float2 x = *reinterpret_cast<const float2*>(xt + tp.off);
            acc[r] = acc[r] + float2v{x.x, x.y} * tp.h;
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int k0 = ((phi0 + r) * M) % L;
        if (k0 < rem) {  // the phases with one tap more: k_0 + L nmin <= 16 M
            const RateTap tp = hrow[r * TS + nmin];
            const float2 x = *reinterpret_cast<const float2*>(xt + tp.off);
            acc[r] = acc[r] + float2v{x.x, x.y} * tp.h;
        }
        ob[(phi0 + r) + (L | 1) * tid] = make_float2(acc[r].x, acc[r].y);
    }
}

template <int F>
__global__ void __launch_bounds__(kNS) rate_ddc_kernel(DdcLaunch A, const RateTap* __restrict__ hp) {
    using Fmt = IqFmt<F>;
    using Raw = typename Fmt::Raw;
    constexpr int PB = Fmt::PB;
    constexpr int NT = kNT, NS = kNS;
    extern __shared__ float2 rate_lds[];
    const int L = A.up, M = A.down;
    const int HC = rate_hist_cols(L), W = rate_row_cols(L), LS = L | 1;
    float2* rot = rate_lds;      // the station's table: (c[p], s[p]), p < N <= kRateMaxN
    float2* xb = rot + kRateMaxN;  // rotated (I', Q') pairs, M polyphase rows of W columns
    float2* ob = xb + M * W;     // the chunk's outputs: lane t's at [LS t, LS t + L)

    const int tid = threadIdx.x, lane = tid & (NT - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / NT);  // wave-uniform: the tap loads stay scalar
    const long long n_out = A.n_out;
    const int CM = NT * L, P = NT * M;  // outputs and wide pairs a chunk
    // chunk indices fit 32 bits for any HBM-resident capture; positions stay 64-bit
    const int n_chunks = (int)((n_out + CM - 1) / CM);
    const int stream = (int)blockIdx.x / A.segs;
    const int seg = (int)blockIdx.x - stream * A.segs;
    const int c0 = (int)((long long)seg * n_chunks / A.segs);
    const int c1 = (int)((long long)(seg + 1) * n_chunks / A.segs);
    if (c0 >= c1) return;

    const uint8_t* in = A.iq;
    const uint8_t* hist = A.hist;
    const long long total = (long long)A.stream_bytes;
    const long long hb = (long long)rate_hist_pairs(L, M) * PB;

    // ---- the station's rotator: table to LDS, phases of this workgroup's first pairs
    const WideStream ws = A.streams[stream];
    const uint32_t N = ws.N, k = ws.k;
    for (uint32_t i = (uint32_t)tid; i < N; i += NS) rot[i] = A.tables[(size_t)stream * kRateMaxN + i];
    const RotatorPhase rp(N, k, A.first_pair, (uint32_t)tid, (uint32_t)NS, (uint32_t)P);
    uint32_t pc = rp.of((long long)c0 * P);  // phase of chunk c's first pair
    __syncthreads();  // table staged

    // ---- prologue: the HC M pairs in front of chunk c0 to buffer pairs [0, HC M); whole units, so an
    // odd count starts one pair early and drops it
    {
        const int hp_pairs = HC * M, hpe = (hp_pairs + 1) & ~1, shift = hpe - hp_pairs;
        for (int j = tid; j < hpe / 2; j += NS) {
            const long long rel = (long long)c0 * P - hpe + 2 * j;
            const Raw w = load_unit_bounded<F>(in, hist, rel * PB, total, hb);
            const uint32_t p0 = rp.of(rel);
            const float4 r = rotate_scaled<F>(w, rot[p0], rot[addmod(p0, k, N)]);
            const int b0 = 2 * j - shift, b1 = b0 + 1;
            if (b0 >= 0) xb[(b0 % M) * W + b0 / M] = make_float2(r.x, r.y);
            xb[(b1 % M) * W + b1 / M] = make_float2(r.z, r.w);
        }
    }

    // ---- where thread t's units of a chunk go: unit u = t + NS l holds chunk pairs 2u, 2u + 1
    const int n_units = P / 2;                 // units a chunk (P is even)
    const int nld = (n_units + NS - 1) / NS;   // loads a thread and chunk (the last one ragged)
    const int col_t = (2 * tid) / M, row_t = 2 * tid - col_t * M;
    const int dcol = (2 * NS) / M, drow = 2 * NS - dcol * M;  // from one load to the next
    // Input prefetch, kK loads ahead: coalesced unit loads, each guarded to the capture (a unit past
    // its end reads as zeros; no output that is stored reads one)
    Raw pf[kK];
    auto fetch = [&](int c, int l0) {
#pragma unroll
        for (int t = 0; t < kK; t++) {
            const int u = tid + (l0 + t) * NS;
            pf[t] = Fmt::zero();
            if (u < n_units) pf[t] = load_unit_bounded<F>(in, hist, ((long long)c * P + 2 * u) * PB, total, hb);
        }
    };
    fetch(c0, 0);

    // the hand-off's read side: element j = tid + NS it of the chunk is phase j mod L of lane j div L
    const int out_t0 = tid / L, out_p0 = tid - out_t0 * L;
    const int out_dt = NS / L, out_dp = NS - out_dt * L;
    // the phases in groups of pg <= kR, dealt to the waves in turn; the number of groups is rounded up
    // to a whole turn, so that the waves carry the same load (L = 24: eight groups of three)
    const int pg_turns = ((L + kR - 1) / kR + kNW - 1) / kNW;
    const int pg = (L + pg_turns * kNW - 1) / (pg_turns * kNW);
    // taps a phase: nmin, and one more for the phases with k_0 < rem
    const int TS = rate_phase_stride(L, M), nmin = rate_taps(M) / L, rem = rate_taps(M) - nmin * L;

    float2* yrow = reinterpret_cast<float2*>(A.y + (size_t)stream * A.y_stride);
    for (int c = c0; c < c1; c++) {
        // ---- stage chunk c: rotate, to the polyphase rows behind the history columns
        {
            uint32_t ph = addmod(pc, rp.tid, N);
            int row = row_t, col = HC + col_t;
            for (int l0 = 0; l0 < nld; l0 += kK) {
                Raw cur[kK];
#pragma unroll
                for (int t = 0; t < kK; t++) cur[t] = pf[t];
                if (l0 + kK < nld) fetch(c, l0 + kK);
#pragma unroll
                for (int t = 0; t < kK; t++) {
                    const int u = tid + (l0 + t) * NS;
                    if (u < n_units) {
                        const float4 r = rotate_scaled<F>(cur[t], rot[ph], rot[addmod(ph, k, N)]);
                        xb[row * W + col] = make_float2(r.x, r.y);
                        const bool last = row + 1 == M;  // the second pair: the next row, or row 0 a column on
                        xb[last ? col + 1 : (row + 1) * W + col] = make_float2(r.z, r.w);
                    }
                    ph = addmod(ph, rp.ld, N);
                    row += drow;
                    col += dcol;
                    if (row >= M) {
                        row -= M;
                        col++;
                    }
                }
            }
            pc = addmod(pc, rp.chunk, N);
        }
        __syncthreads();  // (A) chunk c staged
        if (c + 1 < c1) fetch(c + 1, 0);

        // ---- low-pass, interpolate, decimate: this wave's groups of phases
        for (int phi = wave * pg; phi < L; phi += kNW * pg) {
            switch (std::min(pg, L - phi)) {
                case 1: rate_phases<1>(xb, ob, hp, phi, L, M, TS, nmin, rem, lane); break;
                case 2: rate_phases<2>(xb, ob, hp, phi, L, M, TS, nmin, rem, lane); break;
                case 3: rate_phases<3>(xb, ob, hp, phi, L, M, TS, nmin, rem, lane); break;
                default: rate_phases<4>(xb, ob, hp, phi, L, M, TS, nmin, rem, lane); break;
            }
        }
        __syncthreads();  // (B) all reads of the chunk done, its outputs in the hand-off rows

        // ---- the chunk's last HC columns of every row are the next one's history
        if (c + 1 < c1) {
            for (int j = 0; j < HC; j++)
                for (int r = tid; r < M; r += NS) xb[r * W + j] = xb[r * W + NT + j];
        }
        // ---- coalesced stores: thread tid takes elements tid + NS it
        {
            const long long m0 = (long long)c * CM;
            int t = out_t0, p = out_p0;
            for (int j = tid; j < CM; j += NS) {
                const long long m = m0 + j;
                if (m < n_out) yrow[m] = ob[p + LS * t];
                t += out_dt;
                p += out_dp;
                if (p >= L) {
                    p -= L;
                    t++;
                }
            }
        }
        __syncthreads();  // (C) hand-off rows and history columns read before the next chunk writes them
    }
}

template <int F>
int launch_one(const DdcLaunch& A, int n_streams, hipStream_t s) {
    const size_t lds = rate_lds_bytes(A.up, A.down);
    // > 64 KiB of dynamic LDS for the largest ratios (set per call: per current device)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&rate_ddc_kernel<F>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)rate_lds_bytes(kRateMaxUp, kRateMaxDown)) != hipSuccess)
        return -2;
    hipLaunchKernelGGL((rate_ddc_kernel<F>), dim3(n_streams * A.segs), dim3(kNS), lds, s, A,
                       static_cast<const RateTap*>(A.taps));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int launch_rate_kernel(const DdcLaunch& A, int n_streams, hipStream_t s) {
    switch (A.format) {
        case kIqU8: return launch_one<kIqU8>(A, n_streams, s);
        case kIqS8: return launch_one<kIqS8>(A, n_streams, s);
        case kIqS16: return launch_one<kIqS16>(A, n_streams, s);
        case kIqF32: return launch_one<kIqF32>(A, n_streams, s);
    }
    return -1;
}

}  // namespace fmrx
