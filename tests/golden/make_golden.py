#!/usr/bin/env python3
"""Generate the golden fixtures from the REFERENCE ITSELF (test infrastructure).

Runs the reference's own src/filter.cpp + src/iofunc.cpp (compiled in place from
/root/reference by oracle/Makefile into oracle/_ref/libfmref.so, driven in project.cpp's
sequential block order by oracle/ref_driver.cpp) on deterministic inputs and writes:

  taps.npz              every tap table the receive chain designs (filter.cpp:14-64)
  case_<name>.npz       per-stage outputs of short runs (inputs are regenerated from a recipe
                        and checked against the stored SHA-256)
  hashes.json           SHA-256 of the S16 output of longer runs (10 s of signal)
  rds_<name>.npz        RDS front half (project.cpp:200-271) on a demod input: channel,
                        carrier (PLL input), nco, rds (mixer output)

Inputs (no reference data file holds I/Q — data/samples*.raw are missing blobs):
  synth:<seed>  the repo's deterministic FM-stereo generator (libfmrx fmrx_synth_host,
                integer-only, identical bytes on host and GPU)
  rand:<seed>   uniform random bytes from tests/iqgen.py (splitmix64, numpy-only)
  const128      all bytes 128 (x = 0.0): the reference outputs all-zero PCM

  bench_*               in hashes.json: SHA-256 of the reference PCM over exactly the 1 GiB
                        inputs bench.py times for BASELINE configs[2] and configs[3]
  streams_*             in hashes.json: per-stream PCM SHA-256 of chosen streams of BASELINE
                        configs[4] (256 x 60 s) and of the short RCCL test's 16 x 0.5 s

  unlocked_*            in hashes.json: PCM, mono PCM and final PLL state of mode-0 stereo streams
                        past the trigOffset stick whose loop never locks or slips (random bytes,
                        no pilot, heavy noise) and of a mode-2 stream of > 2^24 PLL steps (the
                        reference hands its PLL the upsampled if_fs, project.cpp:166,348)

  unlocked_c4_*         in hashes.json: the same fields for unlocked streams of BASELINE configs[4]'s
                        length (60 s, 22,500 blocks), which the many-stream tests run among the
                        locked streams of streams_c4_60s

Usage: python tests/golden/make_golden.py [--rds-only | --bench-only | --streams-all | --unlocked-only | --mixed-only]
       (needs /root/reference; not run on the GPU box)
"""
from __future__ import annotations

import hashlib
import json
import os
import platform
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import oracle  # noqa: E402
import iqgen  # noqa: E402

# Small per-stage cases: (name, mode, rf_taps, input recipe, n_blocks, fields stored in full)
ALL = ["demod", "mono_exact", "mono_indep", "pcm", "pcm_mono", "channel", "carrier", "nco",
       "mixer", "stereo", "left", "right", "pll_state"]
CASES = [
    ("m0_rf51_synth", 0, 51, "synth:1", 16, ALL),
    ("m0_rf101_synth", 0, 101, "synth:2", 16, ALL),
    ("m0_rf51_rand", 0, 51, "rand:7", 24, ALL),
    ("m0_rf101_rand", 0, 101, "rand:8", 8, ["demod", "mono_indep", "pcm", "pcm_mono"]),
    ("m0_rf51_const", 0, 51, "const128", 4, ["pcm", "pcm_mono", "demod"]),
    ("m0_rf51_one", 0, 51, "synth:3", 1, ALL),
    ("m1_rf51_synth", 1, 51, "synth:4", 12, ALL),
    ("m1_rf101_rand", 1, 101, "rand:9", 6, ["demod", "mono_indep", "pcm", "pcm_mono"]),
    ("m2_rf51_synth", 2, 51, "synth:5", 2, ["pcm", "pcm_mono", "pll_state"]),
    ("m3_rf51_synth", 3, 51, "synth:6", 1, ["pcm", "pcm_mono", "pll_state"]),
]
# Long runs, hash only: (name, mode, rf_taps, recipe, seconds of signal)
LONG = [
    ("m0_rf51_synth_10s", 0, 51, "synth:11", 10.0),
    ("m0_rf101_synth_10s", 0, 101, "synth:12", 10.0),
    ("m1_rf51_synth_10s", 1, 51, "synth:13", 10.0),
    ("m2_rf51_synth_4s", 2, 51, "synth:14", 4.0),
    ("m3_rf51_synth_8s", 3, 51, "synth:15", 8.0),
    ("m0_rf51_rand_2s", 0, 51, "rand:16", 2.0),
    ("m0_rf51_synth_72s", 0, 51, "synth:17", 72.0),  # PLL trigOffset saturates at 69.9 s
    ("m0_rf51_synth_100s", 0, 51, "synth:18", 100.0),  # 30 s of it stuck (pll_sat.hip's toggle)
]

# The PLL outside the locked regime (filter.cpp:157-171), hash only: (name, mode, rf_taps, recipe,
# seconds of signal).  80 s of mode 0 is 19.2 M steps: past 2^21, 2^22 and the 2^24 stick.
UNLOCKED = [
    ("unlocked_m0_rand_80s", 0, 51, "rand:61", 80.0),       # phase random-walks
    ("unlocked_m0_nopilot_80s", 0, 51, "nopilot:62", 80.0),  # no pilot: the loop runs off frequency
    ("unlocked_m0_noisy_80s", 0, 51, "noisy:63", 80.0),      # heavy noise: cycle slips
    ("unlocked_m2_synth_170b", 2, 51, "synth:64", 72.6),     # 170 blocks, 17.4 M steps at if_fs 35.28 MHz
]

# Unlocked streams of the configs[4] length (60 s: 14.4 M steps, through every runner form below the
# stick), run among the locked synth:<id> streams of streams_c4_60s in one many-stream call.
MIXED = [
    ("unlocked_c4_nopilot_60s", 0, 51, "nopilot:301", 60.0),
    ("unlocked_c4_noisy_60s", 0, 51, "noisy:302", 60.0),
    ("unlocked_c4_rand_60s", 0, 51, "rand:303", 60.0),
    ("unlocked_c4_noisy2_60s", 0, 51, "noisy:304", 60.0),
]


# RDS front half cases: (name, mode, demod source, n_blocks, store outputs in full?)
#   iq:<recipe>  demod = the reference front end on that I/Q (regenerated by the tests with the
#                pinned oracle, checked against the stored demod SHA-256)
#   rds57:<seed> demod synthesized directly (tests/iqgen.py make_rds_demod): mono tone, pilot
#                and a 57 kHz biphase subcarrier; the input itself is stored in the fixture
RDS_CASES = [
    ("m0_rds57", 0, "rds57:1", 24, True),
    ("m0_synth", 0, "iq:synth:41", 16, True),
    ("m1_rand", 1, "iq:rand:42", 8, True),
    ("m2_synth", 2, "iq:synth:43", 2, False),
    ("m3_synth", 3, "iq:synth:44", 1, False),
    ("m0_synth_10s", 0, "iq:synth:45", 1875, False),
]


def rds_demod(ref, mode: int, source: str, nb: int) -> np.ndarray:
    nif = oracle.MODES[mode][1]
    if source.startswith("rds57:"):
        return iqgen.make_rds_demod(int(source[6:]), nb * nif, oracle.MODES[mode][5])
    bb, rf_fs = oracle.MODES[mode][0], oracle.MODES[mode][3]
    iq = iqgen.make(source[3:], nb * bb, rf_fs)
    return ref.run(mode, 51, iq, ["demod"])["demod"]


def make_rds(ref) -> None:
    for name, mode, source, nb, full in RDS_CASES:
        demod = rds_demod(ref, mode, source, nb)
        out = ref.rds(mode, demod)
        arrs = {"demod_sha256": sha(demod)}
        arrs.update({f"{k}_sha256": sha(v) for k, v in out.items()})
        if full:
            arrs.update(out)
        if source.startswith("rds57:") and full:
            arrs["demod"] = demod
        np.savez_compressed(os.path.join(HERE, f"rds_{name}.npz"), mode=mode, source=source,
                            n_blocks=nb, **arrs)
        print(f"rds {name}: {nb} blocks, full={full}")


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# The exact inputs bench.py's other_configs() times (BASELINE configs[2] and configs[3]): the
# reference build's PCM over the same bytes, so the driver-run bench line carries full-size
# parity.  (key, mode, channels, rf_taps, synth seed, pcm field, bench.py workload)
BENCH = [
    ("bench_c2_m0_stereo_gib", 0, 2, 51, 3000, "pcm", "configs[2]"),
    ("bench_c3_m2_mono_gib", 2, 1, 51, 3001, "pcm_mono", "configs[3]"),
]
BENCH_BYTES = 1 << 30  # bench.py STREAM_BYTES
# BASELINE configs[4] (independent mode-0 stereo streams, stream id = synth seed): the reference
# PCM hash of chosen streams, for bench.py's configs[4] leg (256 x 60 s) and the short RCCL test
# (tools/bench_streams.py --streams 16 --seconds 0.5).  (key, seconds, stream ids)
STREAMS = [
    ("streams_c4_60s", 60.0, (0, 127, 128, 255)),  # --streams-all: all 256
    ("streams_c4_short", 0.5, (0, 7, 8, 15)),
]


def make_bench(ref) -> None:
    """Add the bench inputs' hashes to hashes.json (the other entries stay as they are)."""
    path = os.path.join(HERE, "hashes.json")
    with open(path) as f:
        hashes = json.load(f)
    for key, mode, channels, rf_taps, seed, field, cfg in BENCH:
        bb, _, _, rf_fs = oracle.MODES[mode][:4]
        nb = BENCH_BYTES // bb
        iq = iqgen.make(f"synth:{seed}", nb * bb, rf_fs)
        out = ref.run(mode, rf_taps, iq, [field]) if field == "pcm" else {field: ref.run_mono(mode, rf_taps, iq)}
        hashes[key] = {"mode": mode, "channels": channels, "rf_taps": rf_taps, "recipe": f"synth:{seed}",
                       "n_blocks": nb, "bench": cfg, "input_sha256": sha(iq), "field": field,
                       "pcm_sha256": sha(out[field])}
        print(f"bench {key}: {nb} blocks")
        del iq, out
    bb, _, _, rf_fs = oracle.MODES[0][:4]
    for key, secs, sids in STREAMS:
        nb = int(secs * rf_fs * 2 // bb)
        hashes[key] = {"mode": 0, "channels": 2, "rf_taps": 51, "seconds": secs, "n_blocks": nb,
                       "recipe": "synth:<stream id>", "pcm_sha256": {}}
        for sid in sids:
            iq = iqgen.make(f"synth:{sid}", nb * bb, rf_fs)
            hashes[key]["pcm_sha256"][str(sid)] = sha(ref.run(0, 51, iq, ["pcm"])["pcm"])
        print(f"streams {key}: {nb} blocks, streams {sids}")
    with open(path, "w") as f:
        json.dump(hashes, f, indent=1)


def _stream_hash(args):
    """One configs[4] stream through the reference build (a pool worker)."""
    sid, nb = args
    bb, _, _, rf_fs = oracle.MODES[0][:4]
    iq = iqgen.make(f"synth:{sid}", nb * bb, rf_fs)
    return sid, sha(oracle.Reference().run(0, 51, iq, ["pcm"])["pcm"])


def make_streams_all(key: str = "streams_c4_60s", n_streams: int = 256) -> None:
    """Every stream of BASELINE configs[4] (256 x 60 s, stream id = synth seed) through the
    reference build, one process per host core: bench.py's configs[4] leg then checks all of
    them, not a sample (~7 s of reference CPU a stream)."""
    import multiprocessing as mp

    path = os.path.join(HERE, "hashes.json")
    with open(path) as f:
        hashes = json.load(f)
    ent = hashes[key]
    with mp.get_context("spawn").Pool(min(8, os.cpu_count() or 1)) as pool:
        for sid, h in pool.imap_unordered(_stream_hash, [(s, ent["n_blocks"]) for s in range(n_streams)]):
            old = ent["pcm_sha256"].get(str(sid))
            assert old is None or old == h, (sid, old, h)
            ent["pcm_sha256"][str(sid)] = h
            print(f"stream {sid}: {h[:16]}", flush=True)
    ent["pcm_sha256"] = {str(s): ent["pcm_sha256"][str(s)] for s in range(n_streams)}
    with open(path, "w") as f:
        json.dump(hashes, f, indent=1)


def long_entry(ref, mode: int, rf_taps: int, recipe: str, secs: float) -> dict:
    bb, _, _, rf_fs = oracle.MODES[mode][:4]
    nb = int(secs * rf_fs * 2 // bb)
    iq = iqgen.make(recipe, nb * bb, rf_fs)
    out = ref.run(mode, rf_taps, iq, ["pcm", "pcm_mono", "pll_state"])
    return {"mode": mode, "rf_taps": rf_taps, "recipe": recipe, "n_blocks": nb,
            "input_sha256": sha(iq), "pcm_sha256": sha(out["pcm"]),
            "pcm_mono_sha256": sha(out["pcm_mono"]),
            "pll_state_last": [float(v) for v in out["pll_state"][-6:]]}


def make_unlocked(ref, entries=None) -> None:
    """Add the UNLOCKED (or the given) entries to hashes.json (the other entries stay as they are)."""
    path = os.path.join(HERE, "hashes.json")
    with open(path) as f:
        hashes = json.load(f)
    for name, mode, rf_taps, recipe, secs in UNLOCKED if entries is None else entries:
        hashes[name] = long_entry(ref, mode, rf_taps, recipe, secs)
        print(f"unlocked {name}: {hashes[name]['n_blocks']} blocks, PLL {hashes[name]['pll_state_last']}")
    with open(path, "w") as f:
        json.dump(hashes, f, indent=1)


def main() -> None:
    oracle.build(ref=True)
    if "--streams-all" in sys.argv:
        make_streams_all()
        return
    ref = oracle.Reference()
    if "--rds-only" in sys.argv:
        make_rds(ref)
        return
    if "--bench-only" in sys.argv:
        make_bench(ref)
        return
    if "--unlocked-only" in sys.argv:
        make_unlocked(ref)
        return
    if "--mixed-only" in sys.argv:
        make_unlocked(ref, MIXED)
        return
    meta = {"glibc": platform.libc_ver(), "generator": "oracle/_ref/libfmref.so (reference "
            "src/filter.cpp + src/iofunc.cpp, g++ -O3, no -march) via oracle/ref_driver.cpp"}

    taps = {}
    for mode, (bb, nif, na, rf_fs, if_fs, bp_fs, up, down) in oracle.MODES.items():
        for t in (51, 101):
            taps[f"rf_m{mode}_{t}"] = ref.lpf(rf_fs, 100000, t, 1)
        taps[f"audio_m{mode}"] = ref.lpf(if_fs, 16000, 51 * up, up)
        taps[f"ch_m{mode}"] = ref.bpf(bp_fs, 22000.0, 54000.0, 51)
        taps[f"ca_m{mode}"] = ref.bpf(bp_fs, 18500, 19500, 51)
    # primitive-level KATs on tiny random vectors (reference functions called directly)
    rng = iqgen.bytes_("rand:21", 4096)
    x = (rng.astype(np.float32) - 128.0) / 128.0
    prim = {}
    prim["norm_in"] = rng[:512]
    prim["norm_out"] = ref.normalize(rng[:512])
    c = taps["rf_m0_51"]
    st = np.linspace(-0.5, 0.5, 50).astype(np.float32)
    for up, down in ((1, 10), (1, 1), (3, 7)):
        o, s2 = ref.resample(x[:1000], st, c, up, down)
        prim[f"resample_{up}_{down}_out"], prim[f"resample_{up}_{down}_state"] = o, s2
    prim["resample_in"], prim["resample_state"] = x[:1000], st
    d, pv = ref.fmdemod(x[:600], x[600:1200], [0.25, -0.5])
    prim["demod_i"], prim["demod_q"], prim["demod_out"], prim["demod_prev"] = x[:600], x[600:1200], d, pv
    pin = np.sin(2 * np.pi * 19000 / 240000 * np.arange(3000)).astype(np.float32) * 0.1
    po, ps = ref.pll(pin, 19000, 240000, 2, 0, 0.01, [0, 0, 1, 0, 1, 0])
    prim["pll_in"], prim["pll_out"], prim["pll_state"] = pin, po, ps
    np.savez_compressed(os.path.join(HERE, "taps.npz"), **taps, **prim)

    for name, mode, rf_taps, recipe, nb, fields in CASES:
        bb = oracle.MODES[mode][0]
        iq = iqgen.make(recipe, nb * bb, oracle.MODES[mode][3])
        out = ref.run(mode, rf_taps, iq, fields)
        arrs = {k: v for k, v in out.items() if k in fields}
        np.savez_compressed(os.path.join(HERE, f"case_{name}.npz"), mode=mode, rf_taps=rf_taps,
                            recipe=recipe, n_blocks=nb, input_sha256=sha(iq), **arrs)
        print(f"case {name}: {nb} blocks, fields {sorted(arrs)}")

    make_rds(ref)
    hashes = {"meta": meta}
    for name, mode, rf_taps, recipe, secs in LONG:
        hashes[name] = long_entry(ref, mode, rf_taps, recipe, secs)
        print(f"long {name}: {hashes[name]['n_blocks']} blocks")
    with open(os.path.join(HERE, "hashes.json"), "w") as f:
        json.dump(hashes, f, indent=1)
    make_bench(ref)
    make_unlocked(ref)
    make_unlocked(ref, MIXED)


if __name__ == "__main__":
    main()
