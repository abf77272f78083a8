"""tests/stereo_ref.py -- the stereo back end restated for the tests of csrc/stereo.hip.

audio_compose   audio_thread (src/project.cpp:132-196, run_blocks of oracle/fmrx_oracle.c) composed
                block by block from a checker's primitives (bpf, lpf, resample, pll, mixer, lr,
                quant) with the band-pass length as an argument: the oracle's run() and run_audio()
                hard-code 51 taps, the primitives do not.
stereo_plan     what the host launches for one stereo call: launch_bpf_pair, run_stereo_audio,
                stereo_chunks / chunk_begin, launch_stereo_audio_range (csrc/stereo.hip,
                csrc/engine.cpp) and fmrx_audio_block's staging limit (csrc/process.cpp), restated.
special_demod   a demod row with denormals, signed zeros, tiny normals and huge samples in it.

tests/test_gpu_stereo_variants.py runs the GPU against these; tests/test_stereo_variants_host.py
pins them on the CPU."""
from __future__ import annotations

import numpy as np

import iqgen
import oracle

BPF_TAPS = (3, 4, 13, 50, 51, 52, 63, 64)  # the ends of the accepted range, odd and even, around the specialised 51
MONO_DELAY = 5                             # project.cpp:308
PLL0 = (0.0, 0.0, 1.0, 0.0, 1.0, 0.0)      # project.cpp:106-111

# csrc/stereo.hip, csrc/engine.cpp, csrc/ctx.h
BP_TILE = 1024               # kBpTile: outputs a workgroup of bpf_pair_tile_kernel, kBpR = 4 a thread
BP_R = 4
SMALL_AUDIO_BLOCKS = 4       # kSmallAudioBlocks
PINNED_CALL_BYTES = 4 << 20  # kPinnedCallBytes

BPF_TILE_SRC = "bpf_pair_tile_kernel<51, true>"
BPF_TILE = "bpf_pair_tile_kernel<51, false>"
BPF_51 = "bpf_pair_kernel<51>"
BPF_GENERIC = "bpf_pair_generic"
AUDIO_SMALL = "stereo_audio_small_kernel"
AUDIO_TILE = "stereo_audio_tile_kernel"
AUDIO_FRAME = "stereo_audio_kernel"
STATE = "stereo_state_kernel"
NCO = "pll_nco_kernel"
STEREO_KERNELS = {BPF_TILE_SRC, BPF_TILE, BPF_51, BPF_GENERIC, AUDIO_SMALL, AUDIO_TILE, AUDIO_FRAME, STATE, NCO}


# ---- the composition ------------------------------------------------------------------------------------

def fresh_state(mode, bp_taps=51):
    """audio_thread's locals at its start (project.cpp:93-130)."""
    at = 51 * oracle.MODES[mode][6]
    return {"audio": np.zeros(at - 1, np.float32), "mono": np.zeros(MONO_DELAY, np.float32),
            "channel": np.zeros(bp_taps - 1, np.float32), "carrier": np.zeros(bp_taps - 1, np.float32),
            "pll": np.array(PLL0, np.float32)}


def audio_compose(lib, mode, demod, bp_taps=51, state=None, flush=None):
    """audio_thread over whole demod blocks, from lib's primitives (an oracle.Oracle or an
    oracle.Reference), the band-pass pair designed at bp_taps taps.  Returns pcm (R,L interleaved),
    mono_exact, channel, carrier, nco, mixer, stereo, left, right, pll_state (6 floats a block, as
    run_audio) and "state", which continues the stream when passed back in.  `state` is not changed.

    flush: a function applied to the channel and carrier rows of every block before anything reads
    them (the host tests put a flush-to-zero of subnormals there); None is the reference."""
    _, nif, na, _, if_fs, bp_fs, up, down = oracle.MODES[mode]
    at = 51 * up
    # the PLL and the audio low-pass run at if_fs (MODES[mode][4]: the upsampled rate in modes 2 and 3,
    # project.cpp:166), the band-pass pair is designed at bp_fs (MODES[mode][5])
    ch_c = lib.bpf(float(bp_fs), 22000.0, 54000.0, bp_taps)
    ca_c = lib.bpf(float(bp_fs), 18500.0, 19500.0, bp_taps)
    au_c = lib.lpf(float(if_fs), 16000.0, at, up)
    st = {k: np.array(v, np.float32) for k, v in (state or fresh_state(mode, bp_taps)).items()}
    assert st["channel"].size == bp_taps - 1 and st["audio"].size == at - 1
    demod = np.ascontiguousarray(demod, np.float32).reshape(-1)
    nb = demod.size // nif
    assert nb * nif == demod.size, "whole blocks only"
    rows = {k: [] for k in ("pcm", "mono_exact", "channel", "carrier", "nco", "mixer", "stereo", "left", "right",
                            "pll_state")}
    for b in range(nb):
        dem = demod[b * nif:(b + 1) * nif]
        mono, st["audio"] = lib.resample(dem, st["audio"], au_c, up, down)          # project.cpp:146
        shift = np.concatenate([st["mono"], mono[:na - MONO_DELAY]])                # :152-159
        st["mono"] = mono[na - MONO_DELAY:].copy()
        chn, st["channel"] = lib.resample(dem, st["channel"], ch_c, 1, 1)           # :162
        car, st["carrier"] = lib.resample(dem, st["carrier"], ca_c, 1, 1)           # :165
        if flush is not None:
            chn, car = flush(chn), flush(car)
        nco, st["pll"] = lib.pll(car, 19000.0, float(if_fs), 2.0, 0.0, 0.01, st["pll"])  # :166
        mix = lib.mixer(chn, nco)                                                   # :169
        ster, st["audio"] = lib.resample(mix, st["audio"], au_c, up, down)          # :172, the SHARED history
        left, right = lib.lr(shift, ster)                                           # :175
        pcm = np.empty(2 * na, np.int16)                                            # :179-195, R then L
        pcm[0::2] = lib.quant(right)
        pcm[1::2] = lib.quant(left)
        for k, v in (("pcm", pcm), ("mono_exact", mono), ("channel", chn), ("carrier", car), ("nco", nco),
                     ("mixer", mix), ("stereo", ster), ("left", left), ("right", right), ("pll_state", st["pll"].copy())):
            rows[k].append(v)
    out = {k: np.concatenate(v) if v else np.zeros(0, np.int16 if k == "pcm" else np.float32) for k, v in rows.items()}
    out["state"] = st
    return out


def flush_subnormals(x):
    """x with every subnormal replaced by a zero of its sign: what a flushing FIR would hand on."""
    x = np.array(x, np.float32)
    tiny = (x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)
    x[tiny] = np.copysign(np.float32(0.0), x[tiny])
    return x


# ---- the launch plan ---------------------------------------------------------------------------------------

def chunk_begin(n_blocks, k, K, head=8, tail=8):
    """engine.cpp chunk_begin: first block of chunk k of K (k = K: n_blocks)."""
    if K <= 1 or k <= 0:
        return 0 if k <= 0 else n_blocks
    if k >= K:
        return n_blocks
    h, tl = max(1, min(head, 64)), max(1, min(tail, 64))
    return n_blocks * (h + 16 * (k - 1)) // (h + 16 * (K - 2) + tl)


def halo_blocks(mode, rf_taps=51):
    """Blocks of raw I/Q the fused front end's halo spans: mono_halo_bytes (csrc/mono_fused.hip), the largest
    pre-roll chunk of its variants (768 IF samples) plus the RF history, in 16-byte words and one more; u8 pairs.
    Two blocks in modes 0 and 1, one in modes 2 and 3."""
    block_bytes, nif = oracle.MODES[mode][:2]
    pairs = 768 * (block_bytes // 2 // nif) + rf_taps - 1
    return -(-((2 * pairs + 15) // 16 * 16 + 16) // block_bytes)


def chunk_count(mode, n_streams, n_blocks, stereo_chunks=0):
    """engine.cpp stereo_chunks: the knob's count (0: 8 from 16 streams on while a chunk keeps 2^14 IF
    samples, else 1), lowered until no chunk is shorter than the RF halo, which a chunk past the first reads
    from the call's own bytes in front of it."""
    nif = oracle.MODES[mode][1]
    hb = halo_blocks(mode)
    k = 8 if n_streams >= 16 else 1
    if stereo_chunks > 0:
        k = stereo_chunks
    else:
        while k > 1 and n_blocks * nif // k < 16384:
            k -= 1
    while k > 1 and any(chunk_begin(n_blocks, j + 1, k) - chunk_begin(n_blocks, j, k) < hb for j in range(k)):
        k -= 1
    return k


def stereo_plan(mode, bp_taps, bpf_tile, entry, n_streams, n_blocks, stereo_chunks=0):
    """One stereo call of n_blocks blocks a stream through `entry` ("process", "process_device" or
    "audio_block") on a context of the given shape and knobs: the kernels and the route.

    route     "small" (one audio launch carries everything), "serial" (the parallel kernels on the
              context stream) or "pipelined" (run_stereo_pipelined)
    bpf       the band-pass kernel, launched once a chunk
    src       the band-pass launch reads the call's new demod from the pinned staging buffer
    copy      "launch": launch_bpf_pair's 2-D copy feeds a per-output kernel from src; "entry":
              fmrx_audio_block's own 2-D copy to the device (a call past the pinned limit); else None
    audio     the kernels after the PLL runners, in launch order, once each
    chunks    the block boundaries [0, ..., n_blocks]
    bpf_n_if  the IF samples a stream of each band-pass launch; bpf_offset their first sample"""
    assert entry in ("process", "process_device", "audio_block") and n_blocks >= 1
    nif, up = oracle.MODES[mode][1], oracle.MODES[mode][6]
    pinned = entry == "audio_block" and 4 * n_streams * n_blocks * nif <= PINNED_CALL_BYTES
    K = 1 if entry == "audio_block" else chunk_count(mode, n_streams, n_blocks, stereo_chunks)
    tile = bp_taps == 51 and bpf_tile != 0  # kDemodHist = 64 >= 50 always
    src = pinned
    if tile:
        bpf = BPF_TILE_SRC if src else BPF_TILE
    else:
        bpf = BPF_51 if bp_taps == 51 else BPF_GENERIC
    copy = "launch" if src and not tile else "entry" if entry == "audio_block" and not pinned else None
    # launch_stereo_audio_range: modes 0 and 1 at 51 audio taps fit the LDS tile (up = 1, 640 / 768 IF
    # samples and 128 frames a block); modes 2 and 3 take the per-frame kernel
    per_block = AUDIO_TILE if up == 1 else AUDIO_FRAME
    if K > 1:
        route, audio = "pipelined", (NCO, per_block, STATE)
    elif up == 1 and n_blocks <= SMALL_AUDIO_BLOCKS:
        route, audio = "small", (AUDIO_SMALL,)
    else:
        route, audio = "serial", (NCO, per_block, STATE)
    chunks = [chunk_begin(n_blocks, j, K) for j in range(K + 1)]
    return {"route": route, "bpf": bpf, "src": src, "copy": copy, "audio": audio, "chunks": chunks,
            "bpf_n_if": [(b - a) * nif for a, b in zip(chunks, chunks[1:])],
            "bpf_offset": [a * nif for a in chunks[:-1]]}


def plan_kernels(plan):
    return {plan["bpf"], *plan["audio"]}


# ---- special values -----------------------------------------------------------------------------------------

def special_demod(mode, n_blocks, denormals=200):
    """make_rds_demod's row with, from the second block on: `denormals` samples of +-1e-41 alternating in
    sign, 120 of -0.0 (longer than any FIR here), 20 around 1.2e-38 (the smallest normals and the
    largest subnormals) and +-1e30 three samples apart."""
    nif, bp_fs = oracle.MODES[mode][1], oracle.MODES[mode][5]
    assert n_blocks >= 1 and denormals + 120 + 20 + 8 + 96 <= nif
    x = iqgen.make_rds_demod(23 + mode, n_blocks * nif, bp_fs).copy()
    p = nif if n_blocks > 1 else 64
    x[p:p + denormals] = np.float32(1e-41) * np.where(np.arange(denormals) % 2 == 0, 1, -1).astype(np.float32)
    p += denormals + 32
    x[p:p + 120] = np.float32(-0.0)
    p += 120 + 32
    x[p:p + 20] = np.float32(1.2e-38) * (1 + (np.arange(20, dtype=np.float32) - 10) / 64) * np.where(np.arange(20) % 3 == 0, -1, 1)
    p += 20 + 32
    x[p], x[p + 3] = np.float32(1e30), np.float32(-1e30)
    return x.astype(np.float32)
