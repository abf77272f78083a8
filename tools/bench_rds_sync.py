#!/usr/bin/env python3
"""RDS block sync against the back half it sits behind, on device-resident bits, one run.

    python tools/bench_rds_sync.py [--streams 256] [--seconds 10] [--mode 0] [--repeats 5]
                                   [--ab-dir DIR] [--out profiles/rds_sync]

The demod test signal (tests/iqgen.py make_rds_demod) goes through the front half once; each repeat resets
the context, then times fmrx_rds_bits_device on the mixer rows and fmrx_rds_blocks_device on the bits it
just wrote, with HIP events on the context's stream.  A second leg times a tuned fmrx_process_device call
with fmrx_set_rds on and fmrx_set_rds_sync off and on (wall clock, the call's host synchronisation, the copy
of counts and records and the host parse included).  --ab-dir: a directory of bench.py result lines,
parent_*.json and this_*.json from alternating runs of the parent's and this build, folded into the same
profile.  Writes bench_rds_sync.json and bench_rds_sync.md under --out; every number in them was measured on
the GPU they name, by this run or (the bench.py lines) by the runs that wrote --ab-dir.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_rds_decode import bench_ab, event_ms  # noqa: E402


def stage(torch, fm, iqgen, mode, ns, seconds, repeats):
    geo = fm.geometry(fm.default_config(mode, fm.STEREO))
    nif, bp_fs = geo.if_samples, geo.bp_fs
    with fm.Receiver(mode, fm.STEREO, n_streams=ns) as rx:
        g = rx.rds_granule
        nb = int(seconds * bp_fs) // (nif * g) * g
        n = nb * nif
        n_sym = n * 19 // (bp_fs // 2000) // fm.RDS_WINDOW * fm.RDS_BITS_PER_WINDOW
        cap = n_sym // 20  # a transmitter sends a block every 26 bits
        d_in = torch.from_numpy(np.tile(iqgen.make_rds_demod(3, n, bp_fs), (ns, 1))).cuda()
        d_mix = torch.empty_like(d_in)
        d_bits = torch.empty((ns, n_sym), dtype=torch.uint8, device="cuda")
        d_blocks = torch.empty((ns, cap, fm.RDS_BLOCK.itemsize), dtype=torch.uint8, device="cuda")
        d_counts = torch.zeros(ns, dtype=torch.int32, device="cuda")
        stream = torch.cuda.ExternalStream(rx.stream())
        rx.rds_device(d_in.data_ptr(), nb, d_mix.data_ptr())
        d_codes = torch.empty_like(d_bits)
        back = lambda: rx.rds_bits_device(d_mix.data_ptr(), nb, d_bits.data_ptr(), d_codes.data_ptr())
        sync = lambda: rx.rds_blocks_device(d_bits.data_ptr(), n_sym, d_blocks.data_ptr(), cap, d_counts.data_ptr())
        back(), sync(), rx.synchronize()  # warm-up: code objects, buffers sized
        runs = []
        for _ in range(repeats):
            rx.reset()
            runs.append({"bits_ms": round(event_ms(torch, stream, back), 4),
                         "sync_ms": round(event_ms(torch, stream, sync), 4)})
        counts = d_counts.cpu().numpy()
    med = lambda k: statistics.median(r[k] for r in runs)
    sig = n / bp_fs
    return {"workload": f"mode {mode}, {ns} stream(s) x {sig:.3f} s, device rows", "bits_per_stream": n_sym, "runs": runs,
            "bits_ms_median": med("bits_ms"), "sync_ms_median": med("sync_ms"),
            "sync_over_bits": round(med("sync_ms") / med("bits_ms"), 3),
            "sync_stream_seconds_per_s": round(ns * sig / (med("sync_ms") * 1e-3), 1),
            "blocks_accepted_stream0": int(counts[0]), "blocks_accepted_max": int(counts.max())}


def switch(torch, fm, iqgen, mode, ns, repeats):
    """A tuned process_device call of 48 RDS granules a stream with RDS on, the block sync off and on, alternating."""
    with fm.Receiver(mode, fm.MONO, n_streams=ns) as rx:
        nb = 48 * rx.rds_granule
        iq = iqgen.make("synth:3", nb * rx.geo.block_bytes, rx.geo.rf_fs)
        d_iq = torch.from_numpy(np.tile(iq, (ns, 1))).cuda()
        d_pcm = torch.empty((ns, nb * rx.geo.pcm_samples), dtype=torch.int16, device="cuda")
        rx.tune([0] * ns)
        rx.set_rds(True)
        out = {"off_ms": [], "on_ms": []}
        for k in range(2 * (repeats + 1)):
            on = k % 2 == 1
            rx.reset()
            rx.set_rds_sync(on)
            t0 = time.perf_counter()
            rx.process_device(d_iq.data_ptr(), nb, d_pcm.data_ptr())
            rx.synchronize()
            if k >= 2:  # the first pair sizes the buffers
                out["on_ms" if on else "off_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        sig = nb * rx.geo.if_samples / rx.geo.bp_fs
    out.update(workload=f"tuned fmrx_process_device with fmrx_set_rds on, mode {mode} mono, {ns} stream(s) x {sig:.3f} s, wall clock",
               off_ms_median=statistics.median(out["off_ms"]), on_ms_median=statistics.median(out["on_ms"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--switch-streams", type=int, default=16)
    ap.add_argument("--ab-dir")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rds_sync"))
    args = ap.parse_args()
    import torch

    import iqgen

    fm = iqgen.load_fmrx()
    prop = torch.cuda.get_device_properties(0)
    arch = getattr(prop, "gcnArchName", "?").split(":")[0]
    # the runtime names the card generically; gfx950 with 256 CUs is the MI355X
    card = "MI355X" if arch == "gfx950" and prop.multi_processor_count == 256 else "GPU"
    gpu = f"{card} ({torch.cuda.get_device_name(0)}, {arch}, {prop.multi_processor_count} CUs)"
    res = {"gpu": gpu, "measured_on_gpu": True,
           "stage": stage(torch, fm, iqgen, args.mode, args.streams, args.seconds, args.repeats),
           "switch": switch(torch, fm, iqgen, args.mode, args.switch_streams, args.repeats)}
    if args.ab_dir:
        res["bench_py"] = bench_ab(args.ab_dir)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_rds_sync.json"), "w") as f:
        json.dump(res, f, indent=1)
    h, s = res["stage"], res["switch"]
    md = ["## RDS block sync against the back half (bench_rds_sync.json)", "",
          f"Every number below was measured on one {res['gpu']} in one session (the bench.py lines by alternating "
          f"runs just before this tool ran); nothing here is an estimate or a CPU figure.", "",
          f"- {h['workload']} ({h['bits_per_stream']} bits a stream), HIP events on the context's stream, {len(h['runs'])} "
          f"repeats after a warm-up: `fmrx_rds_bits_device` median {h['bits_ms_median']} ms, `fmrx_rds_blocks_device` on the "
          f"bits it wrote median {h['sync_ms_median']} ms: {h['sync_over_bits']} of it, {h['sync_stream_seconds_per_s']} "
          f"stream-seconds a second.  Runs: {h['runs']}.  The test signal's RDS is random bits: "
          f"{h['blocks_accepted_max']} blocks accepted at most a stream.",
          f"- {s['workload']}, `fmrx_set_rds_sync` off and on alternating: median {s['off_ms_median']} ms off "
          f"({min(s['off_ms'])} .. {max(s['off_ms'])}), {s['on_ms_median']} ms on ({min(s['on_ms'])} .. {max(s['on_ms'])})."]
    if "bench_py" in res and "parent_median" in res["bench_py"]:
        b = res["bench_py"]
        md.append(f"- `bench.py --gpus 1 --steps 20 --warmup 3`, parent build and this build alternating, "
                  f"{len(b['parent'])} runs each: parent {[r['MS_per_s'] for r in b['parent']]} MS/s (median "
                  f"{b['parent_median']}, min-to-max spread {b['parent_spread']}), this build "
                  f"{[r['MS_per_s'] for r in b['this']]} (median {b['this_median']}): "
                  f"{'within' if b['within_parent_spread'] else 'OUTSIDE'} the parent's spread.  The headline path "
                  f"(untuned mono) never reaches the RDS code; the switch is off by default.")
    md.append("- Not measured: modes 1 to 3, the host-buffer form, the flush, constants other than the defaults, hardware counters.")
    with open(os.path.join(args.out, "bench_rds_sync.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
