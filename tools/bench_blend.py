#!/usr/bin/env python3
"""Soft stereo on one GPU.

    python tools/bench_blend.py off [--tree DIR] [--repeats 5]          one JSON line
    python tools/bench_blend.py switch [--tree DIR] [--repeats 5]       one JSON line: `on`'s switch leg alone, in DIR's build
    python tools/bench_blend.py on [--repeats 5] [--ab-dir DIR] [--out profiles/blend]

off: a tuned stereo fmrx_process_device call, mode 0, 16 streams x 3.072 s, with the stage off (wall clock, the
call's host synchronisation included), in the build of the repository tree DIR (default: this one) -- the
leg that is run in turn on the parent commit's build and on this one, a process each, to show that off adds
nothing.  on: the same call with fmrx_set_stereo_blend off and on, and with de-emphasis 50 off and on beside
it, alternating; then the apply kernel alone (fmrx_blend_apply_device, HIP events on the context's stream)
over 256 streams x 9.984 s of (R, L) rows, writing PCM and writing floats in place, as GB/s over the bytes
it must move beside a device-to-device copy of the same rows (bench.py's hbm_attainable_GBs, taken here on
the same box).  --ab-dir: the `off` lines of the alternating runs, parent_*.json and this_*.json.  Writes
bench_blend.json and bench_blend.md under --out; every number in them was measured by this run (the `off`
lines by the runs that wrote --ab-dir).
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


def load(tree):
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch

    import iqgen

    return torch, iqgen, iqgen.load_fmrx()


def call_setup(torch, fm, iqgen, ns=16, granules=48):
    rx = fm.Receiver(0, fm.STEREO, n_streams=ns)
    nb = granules * rx.rds_granule
    iq = iqgen.make("synth:3", nb * rx.geo.block_bytes, rx.geo.rf_fs)
    d_iq = torch.from_numpy(np.tile(iq, (ns, 1))).cuda()
    d_pcm = torch.empty((ns, nb * rx.geo.pcm_samples), dtype=torch.int16, device="cuda")
    rx.tune([0] * ns)
    return rx, nb, d_iq, d_pcm


def timed_call(rx, nb, d_iq, d_pcm):
    rx.reset()
    t0 = time.perf_counter()
    rx.process_device(d_iq.data_ptr(), nb, d_pcm.data_ptr())
    rx.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 3)


def leg_off(tree, repeats):
    torch, iqgen, fm = load(tree)
    rx, nb, d_iq, d_pcm = call_setup(torch, fm, iqgen)
    timed_call(rx, nb, d_iq, d_pcm)  # sizes the buffers, loads the code objects
    ms = [timed_call(rx, nb, d_iq, d_pcm) for _ in range(repeats)]
    rx.close()
    return {"leg": "off", "tree": os.path.relpath(os.path.abspath(tree), REPO), "ms": ms, "ms_median": statistics.median(ms),
            "workload": f"tuned stereo fmrx_process_device, mode 0, 16 streams x {nb * 640 / 240000:.3f} s, blend off, wall clock"}


def leg_switch(torch, fm, iqgen, repeats):
    rx, nb, d_iq, d_pcm = call_setup(torch, fm, iqgen)
    kinds = {"off": (False, 0), "blend": (True, 0), "deemph": (False, 50), "blend_deemph": (True, 50)}
    out = {k: [] for k in kinds}
    for r in range(repeats + 1):
        for k, (on, tau) in kinds.items():
            rx.set_stereo_blend(on)
            rx.set_deemphasis(tau)
            ms = timed_call(rx, nb, d_iq, d_pcm)
            if r:  # the first round sizes the buffers
                out[k].append(ms)
    rep = None
    rx.set_stereo_blend(True)
    rx.set_deemphasis(0)
    timed_call(rx, nb, d_iq, d_pcm)
    rep = rx.blend_report(0)
    rx.close()
    res = {"workload": f"tuned stereo fmrx_process_device, mode 0, 16 streams x {nb * 640 / 240000:.3f} s, wall clock, the four settings in turn",
           "ms": out, "median_ms": {k: statistics.median(v) for k, v in out.items()}, "stream0_report": rep}
    m = res["median_ms"]
    res["blend_adds_ms"] = round(m["blend"] - m["off"], 3)
    res["blend_adds_with_deemph_ms"] = round(m["blend_deemph"] - m["deemph"], 3)
    return res


def event_ms(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def copy_gbs(torch, src, reps=20):
    """bench.py's hbm_copy_bandwidth: GB/s (read + written) of a device-to-device copy, median of reps."""
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    del dst
    return round(2 * src.numel() * src.element_size() / statistics.median(times) / 1e9, 1)


def leg_kernel(torch, fm, ns, granules, repeats):
    with fm.Receiver(0, fm.STEREO, n_streams=ns) as rx:
        n = granules * 3072
        g = torch.Generator(device="cuda").manual_seed(5)
        d_x = (torch.rand((ns, n, 2), generator=g, device="cuda", dtype=torch.float32) * 3.0 - 1.5).contiguous()
        d_l = torch.randint(0, 17, (ns, granules + 1), generator=g, device="cuda", dtype=torch.uint8)
        d_p = torch.empty((ns, 2 * n), dtype=torch.int16, device="cuda")
        stream = torch.cuda.ExternalStream(rx.stream())
        forms = {"pcm": lambda: rx.blend_apply(d_x.data_ptr(), n, d_l.data_ptr(), None, d_p.data_ptr()),
                 "floats_in_place": lambda: rx.blend_apply(d_x.data_ptr(), n, d_l.data_ptr(), d_x.data_ptr(), None)}
        out = {}
        for name, run in forms.items():
            run(), rx.synchronize()
            ms = [round(event_ms(torch, stream, run), 4) for _ in range(repeats)]
            moved = ns * n * (8 + (4 if name == "pcm" else 8))
            med = statistics.median(ms)
            out[name] = {"ms": ms, "ms_median": med, "bytes_moved": moved, "GBs": round(moved / (med * 1e-3) / 1e9, 1)}
        hbm = copy_gbs(torch, d_x)
    for v in out.values():
        v["fraction_of_copy"] = round(v["GBs"] / hbm, 3)
    out.update(workload=f"fmrx_blend_apply_device, mode 0, {ns} streams x {n / 48000:.3f} s of (R, L) rows ({ns * n * 8 / 1e9:.3f} GB in), levels uniform in 0..16",
               hbm_attainable_GBs=hbm)
    return out


def ab(ab_dir):
    out = {}
    for who in ("parent", "this"):
        rows = []
        for p in sorted(glob.glob(os.path.join(ab_dir, f"{who}_*.json"))):
            rows += [json.loads(x)["ms_median"] for x in open(p) if x.lstrip().startswith('{"leg"')][:1]
        out[who] = rows
    if out["parent"] and out["this"]:
        out.update(parent_median=statistics.median(out["parent"]), this_median=statistics.median(out["this"]),
                   parent_spread=round(max(out["parent"]) - min(out["parent"]), 3))
        out["within_parent_spread"] = bool(abs(out["this_median"] - out["parent_median"]) <= out["parent_spread"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["off", "switch", "on"])
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--granules", type=int, default=156)
    ap.add_argument("--ab-dir")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "blend"))
    args = ap.parse_args()
    if args.leg == "off":
        print(json.dumps(leg_off(args.tree, args.repeats)))
        return
    if args.leg == "switch":  # the switch leg alone in the build of --tree (tools/bench_quiet.py ab sums the alternating runs up)
        torch, iqgen, fm = load(args.tree)
        res = leg_switch(torch, fm, iqgen, args.repeats)
        print(json.dumps({"leg": "switch", "tree": os.path.relpath(os.path.abspath(args.tree), REPO), **res}))
        return
    torch, iqgen, fm = load(REPO)
    prop = torch.cuda.get_device_properties(0)
    arch = getattr(prop, "gcnArchName", "?").split(":")[0]
    card = "MI355X" if arch == "gfx950" and prop.multi_processor_count == 256 else "GPU"
    res = {"gpu": f"{card} ({torch.cuda.get_device_name(0)}, {arch}, {prop.multi_processor_count} CUs)", "measured_on_gpu": True,
           "switch": leg_switch(torch, fm, iqgen, args.repeats),
           "kernel": leg_kernel(torch, fm, args.streams, args.granules, args.repeats)}
    if args.ab_dir:
        res["off_against_parent"] = ab(args.ab_dir)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_blend.json"), "w") as f:
        json.dump(res, f, indent=1)
    s, k = res["switch"], res["kernel"]
    lines = [f"# Soft stereo on {res['gpu']}", "", f"- {s['workload']}: medians {s['median_ms']} ms; blend adds {s['blend_adds_ms']} ms, "
             f"{s['blend_adds_with_deemph_ms']} ms beside de-emphasis", f"- {k['workload']}: copy {k['hbm_attainable_GBs']} GB/s"]
    for name in ("pcm", "floats_in_place"):
        lines.append(f"  - {name}: {k[name]['ms']} ms, median {k[name]['ms_median']} ms = {k[name]['GBs']} GB/s, {k[name]['fraction_of_copy']} of the copy")
    if args.ab_dir:
        lines.append(f"- blend off against the parent commit's build: {res['off_against_parent']}")
    with open(os.path.join(args.out, "bench_blend.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
