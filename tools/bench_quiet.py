#!/usr/bin/env python3
"""Quieting on one GPU.

    python tools/bench_quiet.py off [--channels 0|1|2] [--tree DIR] [--repeats 5]    one JSON line a channel count (0: both)
    python tools/bench_quiet.py switch [--channels 0|1|2] [--tree DIR] [--repeats 5] one JSON line a channel count
    python tools/bench_quiet.py ab --ab-dir DIR                                      the alternating runs' lines summed up (no GPU)
    python tools/bench_quiet.py on [--repeats 5] [--ab-dir DIR] [--out profiles/quiet]
    python tools/bench_quiet.py kernel-mono [--repeats 5] [--out profiles/quiet]

off: a tuned fmrx_process_device call, mode 0, 16 streams x 3.072 s, mono or stereo, with the stage off (wall
clock, the call's host synchronisation included), in the build of the repository tree DIR (default: this one)
-- the leg that is run in turn on the parent commit's build and on this one, a process each, to show that off
adds nothing (a tree without the stage has no switch to turn: the call is the same).  on: the same calls with
fmrx_set_quieting off and on, alone and beside soft stereo (stereo) and de-emphasis 50, alternating; then the
apply kernel alone (fmrx_quiet_apply_device, HIP events on the context's stream, a warm-up and `repeats` runs)
over 256 streams x 9.984 s of (R, L) rows with levels uniform in 0..16 and with all 16, writing PCM and
writing floats, and in the same run on the same rows fmrx_deemph, fmrx_blend_apply_device and a
device-to-device copy.  switch: those switch legs alone in the build of DIR, for alternating runs against
the parent commit's build of a change to the host code that runs once a call.  --ab-dir: the lines of the alternating runs, parent_*.json and this_*.json (`off`
lines, `switch` lines of this tool and of bench_blend.py, and bench.py result lines).  Writes bench_quiet.json and bench_quiet.md under --out; every number in
them was measured by this run (the alternating lines by the runs that wrote --ab-dir).  kernel-mono: the apply
kernel over the same bytes as rows of a MONO context (contiguous rows; a stereo context's workgroups take one
channel each and read and write every other float), into bench_quiet_kernel_mono.json and .md.
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


def call_setup(torch, fm, iqgen, channels, ns=16, granules=48):
    rx = fm.Receiver(0, fm.STEREO if channels == 2 else fm.MONO, n_streams=ns)
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


def spread(ms):
    return {"ms": ms, "median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def leg_off(torch, iqgen, fm, tree, channels, repeats):
    rx, nb, d_iq, d_pcm = call_setup(torch, fm, iqgen, channels)
    timed_call(rx, nb, d_iq, d_pcm)  # sizes the buffers, loads the code objects
    ms = [timed_call(rx, nb, d_iq, d_pcm) for _ in range(repeats)]
    rx.close()
    return {"leg": "off", "channels": channels, "tree": os.path.relpath(os.path.abspath(tree), REPO), "ms": ms,
            "ms_median": statistics.median(ms),
            "workload": f"tuned {'stereo' if channels == 2 else 'mono'} fmrx_process_device, mode 0, 16 streams x {nb * 640 / 240000:.3f} s, quieting off, wall clock"}


def leg_switch(torch, fm, iqgen, channels, repeats):
    rx, nb, d_iq, d_pcm = call_setup(torch, fm, iqgen, channels)
    kinds = {"off": (False, False, 0), "quiet": (True, False, 0), "deemph": (False, False, 50), "quiet_deemph": (True, False, 50)}
    if channels == 2:
        kinds.update(blend_deemph=(False, True, 50), quiet_blend_deemph=(True, True, 50))
    out = {k: [] for k in kinds}
    for r in range(repeats + 1):
        for k, (quiet, blend, tau) in kinds.items():
            rx.set_quieting(quiet)
            if channels == 2:
                rx.set_stereo_blend(blend)
            rx.set_deemphasis(tau)
            ms = timed_call(rx, nb, d_iq, d_pcm)
            if r:  # the first round sizes the buffers
                out[k].append(ms)
    rx.set_quieting(True)
    rx.set_deemphasis(0)
    timed_call(rx, nb, d_iq, d_pcm)
    rep = rx.quiet_report(0)
    rx.close()
    res = {"workload": f"tuned {'stereo' if channels == 2 else 'mono'} fmrx_process_device, mode 0, 16 streams x {nb * 640 / 240000:.3f} s, wall clock, the settings in turn",
           "runs": {k: spread(v) for k, v in out.items()}, "stream0_report": rep}
    m = {k: v["median"] for k, v in res["runs"].items()}
    res["quiet_adds_ms"] = round(m["quiet"] - m["off"], 3)
    res["quiet_adds_with_deemph_ms"] = round(m["quiet_deemph"] - m["deemph"], 3)
    if channels == 2:
        res["quiet_adds_with_blend_and_deemph_ms"] = round(m["quiet_blend_deemph"] - m["blend_deemph"], 3)
    return res


def event_ms(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def leg_kernel(torch, fm, ns, granules, repeats):
    with fm.Receiver(0, fm.STEREO, n_streams=ns) as rx:
        n = granules * 3072
        g = torch.Generator(device="cuda").manual_seed(5)
        d_x = (torch.rand((ns, n, 2), generator=g, device="cuda", dtype=torch.float32) * 3.0 - 1.5).contiguous()
        d_y = torch.empty_like(d_x)
        d_p = torch.empty((ns, 2 * n), dtype=torch.int16, device="cuda")
        d_uni = torch.randint(0, 17, (ns, granules + 1, 2), generator=g, device="cuda", dtype=torch.uint8)
        d_all = torch.full((ns, granules + 1, 2), 16, device="cuda", dtype=torch.uint8)
        d_bl = torch.randint(0, 17, (ns, granules + 1), generator=g, device="cuda", dtype=torch.uint8)
        d_h = torch.zeros((ns, 2, 63), device="cuda", dtype=torch.float32)
        d_s = torch.zeros(63, device="cuda", dtype=torch.float32)
        stream = torch.cuda.ExternalStream(rx.stream())
        x, y, p = d_x.data_ptr(), d_y.data_ptr(), d_p.data_ptr()
        total = ns * n * 2  # floats of the rows
        forms = {  # name: (the call, bytes it must move)
            "quiet_uniform_pcm": (lambda: rx.quiet_apply(x, n, d_uni.data_ptr(), d_h.data_ptr(), None, p), total * 6),
            "quiet_uniform_floats": (lambda: rx.quiet_apply(x, n, d_uni.data_ptr(), d_h.data_ptr(), y, None), total * 8),
            "quiet_all16_pcm": (lambda: rx.quiet_apply(x, n, d_all.data_ptr(), d_h.data_ptr(), None, p), total * 6),
            "quiet_all16_floats": (lambda: rx.quiet_apply(x, n, d_all.data_ptr(), d_h.data_ptr(), y, None), total * 8),
            "deemph_pcm": (lambda: rx.deemph(x, total, 50, d_s.data_ptr(), None, p), total * 6),
            "deemph_floats": (lambda: rx.deemph(x, total, 50, d_s.data_ptr(), y, None), total * 8),
            "blend_pcm": (lambda: rx.blend_apply(x, n, d_bl.data_ptr(), None, p), total * 6),
            "blend_floats": (lambda: rx.blend_apply(x, n, d_bl.data_ptr(), y, None), total * 8),
            "copy": (lambda: d_y.copy_(d_x), total * 8),
        }
        out = {}
        for name, (run, moved) in forms.items():
            st = torch.cuda.current_stream() if name == "copy" else stream
            run(), rx.synchronize(), torch.cuda.synchronize()
            ms = [round(event_ms(torch, st, run), 4) for _ in range(repeats)]
            med = statistics.median(ms)
            out[name] = {"ms": ms, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "bytes_moved": moved,
                         "GBs": round(moved / (med * 1e-3) / 1e9, 1)}
    m = {k: v["ms_median"] for k, v in out.items()}
    res = {"workload": f"mode 0, {ns} streams x {n / 48000:.3f} s of (R, L) rows ({total * 4 / 1e9:.3f} GB in), HIP events, a warm-up and {repeats} runs each",
           "forms": out,
           "quiet_uniform_over_deemph_plus_blend": {k: round(m[f"quiet_uniform_{k}"] / (m[f"deemph_{k}"] + m[f"blend_{k}"]), 3) for k in ("pcm", "floats")},
           "quiet_all16_floats_over_copy": round(m["quiet_all16_floats"] / m["copy"], 3)}
    return res


def leg_kernel_mono(torch, fm, ns, granules, repeats):
    """The same bytes as leg_kernel's rows on a MONO context (2 x granules a stream): contiguous rows, where a
    stereo context's workgroups read and write every other float."""
    with fm.Receiver(0, fm.MONO, n_streams=ns) as rx:
        n = 2 * granules * 3072
        g = torch.Generator(device="cuda").manual_seed(5)
        d_x = (torch.rand((ns, n), generator=g, device="cuda", dtype=torch.float32) * 3.0 - 1.5).contiguous()
        d_y = torch.empty_like(d_x)
        d_p = torch.empty((ns, n), dtype=torch.int16, device="cuda")
        d_uni = torch.randint(0, 17, (ns, 2 * granules + 1, 2), generator=g, device="cuda", dtype=torch.uint8)
        d_all = torch.full((ns, 2 * granules + 1, 2), 16, device="cuda", dtype=torch.uint8)
        d_h = torch.zeros((ns, 1, 63), device="cuda", dtype=torch.float32)
        stream = torch.cuda.ExternalStream(rx.stream())
        x, y, p, total = d_x.data_ptr(), d_y.data_ptr(), d_p.data_ptr(), ns * n
        forms = {
            "quiet_uniform_pcm": (lambda: rx.quiet_apply(x, n, d_uni.data_ptr(), d_h.data_ptr(), None, p), total * 6),
            "quiet_uniform_floats": (lambda: rx.quiet_apply(x, n, d_uni.data_ptr(), d_h.data_ptr(), y, None), total * 8),
            "quiet_all16_pcm": (lambda: rx.quiet_apply(x, n, d_all.data_ptr(), d_h.data_ptr(), None, p), total * 6),
            "quiet_all16_floats": (lambda: rx.quiet_apply(x, n, d_all.data_ptr(), d_h.data_ptr(), y, None), total * 8),
            "copy": (lambda: d_y.copy_(d_x), total * 8),
        }
        out = {}
        for name, (run, moved) in forms.items():
            st = torch.cuda.current_stream() if name == "copy" else stream
            run(), rx.synchronize(), torch.cuda.synchronize()
            ms = [round(event_ms(torch, st, run), 4) for _ in range(repeats)]
            med = statistics.median(ms)
            out[name] = {"ms": ms, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "bytes_moved": moved,
                         "GBs": round(moved / (med * 1e-3) / 1e9, 1)}
    return {"workload": f"mode 0 MONO, {ns} streams x {n / 48000:.3f} s of rows ({total * 4 / 1e9:.3f} GB in), HIP events, a warm-up and {repeats} runs each",
            "forms": out, "quiet_all16_floats_over_copy": round(out["quiet_all16_floats"]["ms_median"] / out["copy"]["ms_median"], 3)}


def write_kernel_mono(res, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_quiet_kernel_mono.json"), "w") as f:
        json.dump(res, f, indent=1)
    k = res["kernel_mono"]
    lines = [f"# Quieting's apply kernel on mono rows, {res['gpu']}", "", f"- {k['workload']}:"]
    for name, v in k["forms"].items():
        lines.append(f"  - {name}: median {v['ms_median']} ms [{v['ms_min']} .. {v['ms_max']}] = {v['GBs']} GB/s of the bytes it must move")
    lines.append(f"  - quieting (all 16, floats) over the copy: {k['quiet_all16_floats_over_copy']}")
    with open(os.path.join(out_dir, "bench_quiet_kernel_mono.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


def ab(ab_dir):
    """The alternating runs' lines by kind: the `off` legs (mono, stereo) in ms, bench.py's headline value."""
    out = {}
    for who in ("parent", "this"):
        for p in sorted(glob.glob(os.path.join(ab_dir, f"{who}_*.json"))):
            for line in open(p):
                line = line.strip()
                if not line.startswith("{"):
                    continue
                try:
                    row = json.loads(line)
                except ValueError:
                    continue
                if row.get("leg") == "switch":  # this tool's lines hold `runs`, bench_blend.py's `median_ms`
                    name = "blend_tool_stereo" if "median_ms" in row else "stereo" if row["channels"] == 2 else "mono"
                    for k, v in (row.get("median_ms") or {k: r["median"] for k, r in row["runs"].items()}).items():
                        out.setdefault(f"switch_{name}_{k}_ms", {}).setdefault(who, []).append(v)
                elif row.get("leg") == "off":
                    out.setdefault(f"off_{'stereo' if row['channels'] == 2 else 'mono'}_ms", {}).setdefault(who, []).append(row["ms_median"])
                elif "value" in row and "metric" in row:
                    out.setdefault(f"bench_py_{row.get('unit', 'value')}", {}).setdefault(who, []).append(row["value"])
    for v in out.values():
        if v.get("parent") and v.get("this"):
            v.update(parent_median=statistics.median(v["parent"]), this_median=statistics.median(v["this"]),
                     parent_min=min(v["parent"]), parent_max=max(v["parent"]))
            v["this_median_within_parent_min_max"] = bool(v["parent_min"] <= v["this_median"] <= v["parent_max"])
            v["difference_within_parent_spread"] = bool(abs(v["this_median"] - v["parent_median"]) <= v["parent_max"] - v["parent_min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["off", "switch", "ab", "on", "kernel-mono"])
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--channels", type=int, default=0, choices=[0, 1, 2])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--granules", type=int, default=156)
    ap.add_argument("--ab-dir")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "quiet"))
    args = ap.parse_args()
    if args.leg == "off":
        loaded = load(args.tree)
        for channels in ((1, 2) if args.channels == 0 else (args.channels,)):
            print(json.dumps(leg_off(*loaded, args.tree, channels, args.repeats)), flush=True)
        return
    if args.leg == "switch":
        torch, iqgen, fm = load(args.tree)
        for channels in ((1, 2) if args.channels == 0 else (args.channels,)):
            res = leg_switch(torch, fm, iqgen, channels, args.repeats)
            print(json.dumps({"leg": "switch", "channels": channels, "tree": os.path.relpath(os.path.abspath(args.tree), REPO), **res}), flush=True)
        return
    if args.leg == "ab":
        print(json.dumps(ab(args.ab_dir), indent=1))
        return
    torch, iqgen, fm = load(REPO)
    prop = torch.cuda.get_device_properties(0)
    arch = getattr(prop, "gcnArchName", "?").split(":")[0]
    card = "MI355X" if arch == "gfx950" and prop.multi_processor_count == 256 else "GPU"
    gpu = f"{card} ({torch.cuda.get_device_name(0)}, {arch}, {prop.multi_processor_count} CUs)"
    if args.leg == "kernel-mono":
        res = {"gpu": gpu, "measured_on_gpu": True, "kernel_mono": leg_kernel_mono(torch, fm, args.streams, args.granules, args.repeats)}
        write_kernel_mono(res, args.out)
        print(json.dumps(res))
        return
    res = {"gpu": gpu, "measured_on_gpu": True,
           "switch_mono": leg_switch(torch, fm, iqgen, 1, args.repeats), "switch_stereo": leg_switch(torch, fm, iqgen, 2, args.repeats),
           "kernel": leg_kernel(torch, fm, args.streams, args.granules, args.repeats)}
    if args.ab_dir:
        res["off_against_parent"] = ab(args.ab_dir)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_quiet.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = [f"# Quieting on {res['gpu']}", "", "Every number below was measured by one run of `tools/bench_quiet.py on` (the alternating "
             "lines by the runs that wrote its --ab-dir); [min .. max] is the spread of the runs.", ""]
    for key in ("switch_mono", "switch_stereo"):
        s = res[key]
        lines.append(f"- {s['workload']}:")
        for k, v in s["runs"].items():
            lines.append(f"  - {k}: median {v['median']} ms [{v['min']} .. {v['max']}]")
        lines.append("  - quieting adds " + ", ".join(f"{v} ms ({k[len('quiet_adds'):-3].strip('_').replace('_', ' ') or 'alone'})"
                                                    for k, v in s.items() if k.startswith("quiet_adds")))
    k = res["kernel"]
    lines.append(f"- the kernels alone, {k['workload']}:")
    for name, v in k["forms"].items():
        lines.append(f"  - {name}: median {v['ms_median']} ms [{v['ms_min']} .. {v['ms_max']}] = {v['GBs']} GB/s of the bytes it must move")
    lines.append(f"  - quieting (uniform levels) over de-emphasis + blend: {k['quiet_uniform_over_deemph_plus_blend']}; "
                 f"quieting (all 16, floats) over the copy: {k['quiet_all16_floats_over_copy']}")
    if args.ab_dir:
        for name, v in res["off_against_parent"].items():
            lines.append(f"- stage off against the parent commit's build, {name}: {v}")
    with open(os.path.join(args.out, "bench_quiet.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
