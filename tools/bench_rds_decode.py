#!/usr/bin/env python3
"""RDS back half against the front half, on device-resident rows, one run.

    python tools/bench_rds_decode.py [--streams 256] [--seconds 10] [--mode 0] [--repeats 5]
                                     [--ab-dir DIR] [--out profiles/rds_decode]

The demod test signal (tests/iqgen.py make_rds_demod) is uploaded once for every stream.  Each repeat
resets the context, then times fmrx_rds_device (front half: two 51-tap band-passes, the serial PLL, the
mixer) and fmrx_rds_bits_device (back half: 19/down resampler of 101 taps a phase, signs, windows,
symbols, syndromes) on the rows the front half just wrote, with HIP events on the context's stream.
A second leg times a tuned fmrx_process_device call with fmrx_set_rds off and on (wall clock, the
call's host synchronisation included).  --ab-dir: a directory of bench.py result lines, parent_*.json
and this_*.json from alternating runs of the parent's and this build, folded into the same profile.
Writes bench_rds_decode.json and bench_rds_decode.md under --out; every number in them was measured
on the GPU they name, by this run or (the bench.py lines) by the runs that wrote --ab-dir.
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))


def event_ms(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def halves(torch, fm, iqgen, mode, ns, seconds, repeats):
    geo = fm.geometry(fm.default_config(mode, fm.STEREO))
    nif, bp_fs = geo.if_samples, geo.bp_fs
    with fm.Receiver(mode, fm.STEREO, n_streams=ns) as rx:
        g = rx.rds_granule
        nb = int(seconds * bp_fs) // (nif * g) * g
        n = nb * nif
        n_out = n * 19 // (bp_fs // 2000)
        n_sym = n_out // fm.RDS_WINDOW * fm.RDS_BITS_PER_WINDOW
        d_in = torch.from_numpy(np.tile(iqgen.make_rds_demod(3, n, bp_fs), (ns, 1))).cuda()
        d_mix = torch.empty_like(d_in)
        d_bits = torch.empty((ns, n_sym), dtype=torch.uint8, device="cuda")
        d_codes = torch.empty_like(d_bits)
        stream = torch.cuda.ExternalStream(rx.stream())
        front = lambda: rx.rds_device(d_in.data_ptr(), nb, d_mix.data_ptr())
        back = lambda: rx.rds_bits_device(d_mix.data_ptr(), nb, d_bits.data_ptr(), d_codes.data_ptr())
        front(), back(), rx.synchronize()  # warm-up: code objects, buffers sized
        runs = []
        for _ in range(repeats):
            rx.reset()
            runs.append({"front_ms": round(event_ms(torch, stream, front), 3),
                         "back_ms": round(event_ms(torch, stream, back), 3)})
        codes = d_codes.cpu().numpy()
    med = lambda k: statistics.median(r[k] for r in runs)
    sig = n / bp_fs
    return {"workload": f"mode {mode}, {ns} stream(s) x {sig:.3f} s, device rows", "runs": runs,
            "front_ms_median": med("front_ms"), "back_ms_median": med("back_ms"),
            "back_over_front": round(med("back_ms") / med("front_ms"), 3),
            "products_ratio_back_over_front_filters": round(38000 * 101 / (bp_fs * 102), 3),
            "back_stream_seconds_per_s": round(ns * sig / (med("back_ms") * 1e-3), 1),
            "blocks_matched_stream0": int(np.count_nonzero(codes[0]))}


def switch(torch, fm, iqgen, mode, ns, repeats):
    """A tuned process_device call of 48 RDS granules a stream, fmrx_set_rds off and on, alternating."""
    with fm.Receiver(mode, fm.MONO, n_streams=ns) as rx:
        nb = 48 * rx.rds_granule
        iq = iqgen.make("synth:3", nb * rx.geo.block_bytes, rx.geo.rf_fs)
        d_iq = torch.from_numpy(np.tile(iq, (ns, 1))).cuda()
        d_pcm = torch.empty((ns, nb * rx.geo.pcm_samples), dtype=torch.int16, device="cuda")
        rx.tune([0] * ns)
        out = {"off_ms": [], "on_ms": []}
        for k in range(2 * (repeats + 1)):
            on = k % 2 == 1
            rx.reset()
            rx.set_rds(on)
            t0 = time.perf_counter()
            rx.process_device(d_iq.data_ptr(), nb, d_pcm.data_ptr())
            rx.synchronize()
            if k >= 2:  # the first pair sizes the buffers
                out["on_ms" if on else "off_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        sig = nb * rx.geo.if_samples / rx.geo.bp_fs
    out.update(workload=f"tuned fmrx_process_device, mode {mode} mono, {ns} stream(s) x {sig:.3f} s, wall clock",
               off_ms_median=statistics.median(out["off_ms"]), on_ms_median=statistics.median(out["on_ms"]))
    return out


def bench_ab(ab_dir):
    """bench.py result lines of alternating runs: medians and the parent's own spread."""
    out = {}
    for who in ("parent", "this"):
        rows = []
        for p in sorted(glob.glob(os.path.join(ab_dir, f"{who}_*.json"))):
            lines = [json.loads(x) for x in open(p) if x.lstrip().startswith("{")]
            rows += [{"MS_per_s": x["value"], "ms_per_step": x.get("ms_per_step")} for x in lines if "value" in x][:1]
        out[who] = rows
    if out["parent"] and out["this"]:
        pv = [r["MS_per_s"] for r in out["parent"]]
        tv = [r["MS_per_s"] for r in out["this"]]
        out.update(parent_median=statistics.median(pv), this_median=statistics.median(tv),
                   parent_spread=round(max(pv) - min(pv), 1))
        out["within_parent_spread"] = bool(out["parent_median"] - out["this_median"] <= out["parent_spread"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--switch-streams", type=int, default=16)
    ap.add_argument("--ab-dir")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rds_decode"))
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
           "halves": halves(torch, fm, iqgen, args.mode, args.streams, args.seconds, args.repeats),
           "switch": switch(torch, fm, iqgen, args.mode, args.switch_streams, args.repeats)}
    if args.ab_dir:
        res["bench_py"] = bench_ab(args.ab_dir)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_rds_decode.json"), "w") as f:
        json.dump(res, f, indent=1)
    h, s = res["halves"], res["switch"]
    md = [f"## RDS back half against the front half (bench_rds_decode.json)", "",
          f"Every number below was measured on one {res['gpu']} in one session (the bench.py lines by alternating "
          f"runs just before this tool ran); nothing here is an estimate or a CPU figure.", "",
          f"- {h['workload']}, HIP events on the context's stream, {len(h['runs'])} repeats after a warm-up: front half "
          f"(`fmrx_rds_device`) median {h['front_ms_median']} ms, back half (`fmrx_rds_bits_device`) median "
          f"{h['back_ms_median']} ms: {h['back_over_front']} of the front half (by products against the front half's "
          f"two filters alone: {h['products_ratio_back_over_front_filters']}).  The back half runs "
          f"{h['back_stream_seconds_per_s']} stream-seconds a second.",
          f"- {s['workload']}, `fmrx_set_rds` off and on alternating: median {s['off_ms_median']} ms off, "
          f"{s['on_ms_median']} ms on (the front half, the back half, the copy of bits and codes and the host parse)."]
    if "bench_py" in res and "parent_median" in res["bench_py"]:
        b = res["bench_py"]
        md.append(f"- `bench.py --gpus 1 --steps 20 --warmup 3`, parent build and this build alternating, "
                  f"{len(b['parent'])} runs each: parent median {b['parent_median']} MS/s (min-to-max spread "
                  f"{b['parent_spread']}), this build {b['this_median']} MS/s: "
                  f"{'within' if b['within_parent_spread'] else 'OUTSIDE'} the parent's spread.  The headline path "
                  f"(untuned mono) never reaches the RDS code; the switch is off by default.")
    md.append("- Not measured: modes 1 to 3, the host-buffer twins, hardware counters.")
    with open(os.path.join(args.out, "bench_rds_decode.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
