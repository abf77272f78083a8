#!/usr/bin/env python3
"""What FM de-emphasis costs, on device-resident buffers, one run.

    python tools/bench_deemph.py [--parent-pkg DIR] [--ab-dir DIR] [--repeats 15]
                                 [--stereo-streams 256] [--stereo-seconds 10] [--out profiles/deemph]

On path: mode-0 mono, 101 RF taps, one device-resident GiB (bench.py's input), fmrx_process_device with
fmrx_set_deemphasis(75) against the yardstick: the parent commit's fmrx_process_device on the same bytes
(--parent-pkg: the package directory of a built checkout of the parent, loaded beside this build) or,
without it, this build with de-emphasis off (the result says which).  The legs alternate; each call is
timed by a host clock around the call and the context's synchronise; median of --repeats after a warm-up
of three calls and at least a second a leg.  The ratio is gated at 1.25.  The kernel's own time: HIP event
pairs around fmrx_deemph on one row of the same 10.7 M frames.  One stereo leg: --stereo-streams streams x
--stereo-seconds s of mode 0, against the same yardstick.  --ab-dir: bench.py result lines parent_*.json
and this_*.json of alternating runs (the off path), folded into the same profile.  Writes
bench_deemph.json and bench_deemph.md under --out; every number in them was measured on the GPU they name.
"""
import argparse
import glob
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

STREAM_BYTES = 1 << 30
GATE = 1.25


def load_parent(pkg):
    """The parent's binding from its own package directory (its libfmrx.so beside it)."""
    spec = importlib.util.spec_from_file_location("fmrx_parent", os.path.join(pkg, "fmrx.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.lib()
    return mod


def timed(call, sync):
    t0 = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t0) * 1e3


def alternate(legs, repeats, min_warm_s=1.0):
    """legs: name -> (call, sync[, prepare]); prepare runs untimed in front of each call.  Warm-up every
    leg, then `repeats` rounds of every leg in turn."""
    legs = {k: (v + (lambda: None,))[:3] for k, v in legs.items()}
    for call, sync, prep in legs.values():
        prep()
        t0, k = time.perf_counter(), 0
        while k < 3 or time.perf_counter() - t0 < min_warm_s:
            call()
            sync()
            k += 1
    ms = {name: [] for name in legs}
    for _ in range(repeats):
        for name, (call, sync, prep) in legs.items():
            prep()
            ms[name].append(round(timed(call, sync), 4))
    return ms


def summary(ms):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": v} for k, v in ms.items()}


def on_path(torch, fm, parent, repeats, contexts):
    """`contexts` contexts a build, created in pairs (this, this, parent, parent, ...); every context of
    this build runs both off and on (fmrx_set_deemphasis between the timed calls).  The fused kernel runs
    at one of two speeds, about 0.55 and 0.74 ms, that stays with a leg for the whole run and has nothing
    to do with the build (the parent's own contexts show both), so one context a build compares the modes,
    not the builds.  The gated ratio is therefore like against like: the fastest on leg over the fastest
    yardstick leg; the means over the contexts and on / off on the same context are recorded beside it."""
    rxs, pars = [], []
    for k in range(0, contexts, 2):
        rxs += [fm.Receiver(0, fm.MONO, rf_taps=101) for _ in range(min(2, contexts - k))]
        if parent:
            pars += [parent.Receiver(0, parent.MONO, rf_taps=101) for _ in range(min(2, contexts - k))]
    rx = rxs[0]
    bb, na = rx.geo.block_bytes, rx.geo.audio_frames
    nb = STREAM_BYTES // bb
    d_iq = torch.empty(STREAM_BYTES, dtype=torch.uint8, device="cuda")
    pcm = {k: torch.empty(nb * na, dtype=torch.int16, device="cuda") for k in ("on", "off", "parent")}
    torch.cuda.synchronize()
    rx.synth_device(1000, 0, STREAM_BYTES // 2, d_iq.data_ptr())
    rx.synchronize()

    def leg(r, key, tau=None):
        def call():
            r.process_device(d_iq.data_ptr(), nb, pcm[key].data_ptr())
        # this build's contexts: the leg's setting, outside the timed window (it drains the stream)
        return (call, r.synchronize) if tau is None else (call, r.synchronize, lambda: r.set_deemphasis(tau))

    legs = {}
    for i, r in enumerate(rxs):
        legs[f"this{i}_off"] = leg(r, "off", 0)
        legs[f"this{i}_on"] = leg(r, "on", 75)
    for i, r in enumerate(pars):
        legs[f"parent{i}"] = leg(r, "parent")
    res = summary(alternate(legs, repeats))
    mean = lambda names: statistics.mean(res[n]["median_ms"] for n in names)
    on = mean([f"this{i}_on" for i in range(len(rxs))])
    off = mean([f"this{i}_off" for i in range(len(rxs))])
    yard = mean([f"parent{i}" for i in range(len(pars))]) if pars else off
    fast = lambda names: min(res[n]["median_ms"] for n in names)
    on_fast = fast([f"this{i}_on" for i in range(len(rxs))])
    yard_fast = fast([f"parent{i}" for i in range(len(pars))] if pars else [f"this{i}_off" for i in range(len(rxs))])
    ratio = on_fast / yard_fast
    out = {"workload": f"mode 0 mono, 101 RF taps, {nb} blocks ({nb * bb} bytes) device-resident, fmrx_process_device",
           "yardstick": "the parent commit's build" if pars else "this build with de-emphasis off (no --parent-pkg)",
           "contexts_a_build": len(rxs), "legs": res, "on_ms": round(on, 4), "this_build_off_ms": round(off, 4),
           "yardstick_ms": round(yard, 4), "ratio_of_means": round(on / yard, 4),
           "on_fastest_ms": on_fast, "yardstick_fastest_ms": yard_fast, "ratio_on_over_yardstick": round(ratio, 4),
           "ratio_on_over_off_same_context": round(statistics.mean(
               res[f"this{i}_on"]["median_ms"] / res[f"this{i}_off"]["median_ms"] for i in range(len(rxs))), 4),
           "gate": GATE, "gate_ok": bool(ratio <= GATE), "audio_frames": nb * na}
    if pars:  # off is the parent's bits
        out["off_equals_parent_pcm"] = bool(torch.equal(pcm["off"], pcm["parent"]))
    rx.set_deemphasis(75)
    rest = rxs[1:] + pars
    # the kernel alone: one row of the call's frames through the primitive, HIP events on the context stream
    n = nb * na
    d_x = torch.rand(n, dtype=torch.float32, device="cuda") - 0.5
    d_st = torch.zeros(63, dtype=torch.float32, device="cuda")
    stream = torch.cuda.ExternalStream(rx.stream())
    torch.cuda.synchronize()
    ev = []
    for k in range(3 + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        rx.deemph(d_x.data_ptr(), n, 75, d_st.data_ptr(), None, pcm["on"].data_ptr())
        b.record(stream)
        b.synchronize()
        if k >= 3:
            ev.append(round(a.elapsed_time(b), 4))
    med = statistics.median(ev)
    out["kernel"] = {"what": f"fmrx_deemph on one row of {n} floats (the launch and the 252-byte state copy behind it), HIP events",
                     "median_ms": med, "min_ms": min(ev), "max_ms": max(ev), "runs_ms": ev,
                     "bytes": 6 * n, "GB_per_s": round(6 * n / (med * 1e-3) / 1e9, 1),
                     "rounded_ops": 128 * n, "Tops_per_s": round(128 * n / (med * 1e-3) / 1e12, 2)}
    for r in [rx] + rest:
        r.close()
    return out


def stereo(torch, fm, parent, ns, seconds, repeats):
    geo = fm.geometry(fm.default_config(0, fm.STEREO))
    nb = int(seconds * geo.rf_fs * 2) // geo.block_bytes
    rx = fm.Receiver(0, fm.STEREO, n_streams=ns)
    rx.set_deemphasis(75)
    ry = parent.Receiver(0, parent.STEREO, n_streams=ns) if parent else fm.Receiver(0, fm.STEREO, n_streams=ns)
    d_iq = torch.empty((ns, nb * geo.block_bytes), dtype=torch.uint8, device="cuda")
    d_pcm = torch.empty((ns, nb * geo.pcm_samples), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rx.synth_device_streams(list(range(1, ns + 1)), 0, nb * geo.iq_pairs, d_iq.data_ptr(), nb * geo.block_bytes)
    rx.synchronize()

    def leg(r):
        def call():
            r.reset()
            r.process_device(d_iq.data_ptr(), nb, d_pcm.data_ptr())
        return call, r.synchronize

    res = summary(alternate({"on_75us": leg(rx), "yardstick": leg(ry)}, repeats, min_warm_s=0.0))
    rx.close()
    ry.close()
    return {"workload": f"mode 0 stereo, {ns} streams x {nb * geo.iq_pairs / geo.rf_fs:.3f} s, one fmrx_process_device call after a reset",
            "yardstick": "the parent commit's build" if parent else "this build with de-emphasis off",
            "legs": res, "ratio_on_over_yardstick": round(res["on_75us"]["median_ms"] / res["yardstick"]["median_ms"], 4)}


def bench_ab(ab_dir):
    """bench.py result lines of alternating runs: medians and the parent's own spread."""
    out = {}
    for who in ("parent", "this"):
        rows = []
        for p in sorted(glob.glob(os.path.join(ab_dir, f"{who}_*.json"))):
            lines = [json.loads(x) for x in open(p) if x.lstrip().startswith("{")]
            rows += [x["value"] for x in lines if "value" in x][:1]
        out[who] = rows
    if out["parent"] and out["this"]:
        out.update(parent_median=statistics.median(out["parent"]), this_median=statistics.median(out["this"]),
                   parent_min=min(out["parent"]), parent_max=max(out["parent"]))
        out["this_median_within_parent_min_max"] = bool(out["parent_min"] <= out["this_median"] <= out["parent_max"])
        out["this_median_not_below_parent_min"] = bool(out["this_median"] >= out["parent_min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg")
    ap.add_argument("--ab-dir")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--contexts", type=int, default=4, help="contexts a build in the on-path leg")
    ap.add_argument("--stereo-streams", type=int, default=256)
    ap.add_argument("--stereo-seconds", type=float, default=10.0)
    ap.add_argument("--stereo-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deemph"))
    args = ap.parse_args()
    import torch

    import iqgen

    if not torch.cuda.is_available():
        sys.exit("bench_deemph.py: no GPU (there is no CPU path to time)")
    fm = iqgen.load_fmrx()
    parent = load_parent(args.parent_pkg) if args.parent_pkg else None
    prop = torch.cuda.get_device_properties(0)
    arch = getattr(prop, "gcnArchName", "?").split(":")[0]
    card = "MI355X" if arch == "gfx950" and prop.multi_processor_count == 256 else "GPU"
    res = {"gpu": f"{card} ({torch.cuda.get_device_name(0)}, {arch}, {prop.multi_processor_count} CUs)", "measured_on_gpu": True,
           "on_path": on_path(torch, fm, parent, args.repeats, args.contexts)}
    if args.stereo_streams > 0:
        res["stereo"] = stereo(torch, fm, parent, args.stereo_streams, args.stereo_seconds, args.stereo_repeats)
    if args.ab_dir:
        res["bench_py"] = bench_ab(args.ab_dir)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_deemph.json"), "w") as f:
        json.dump(res, f, indent=1)
    o, k = res["on_path"], res["on_path"]["kernel"]
    L = o["legs"]
    md = ["## FM de-emphasis (bench_deemph.json)", "",
          f"Measured on one {res['gpu']}; nothing here is an estimate or a CPU figure.", "",
          f"- On path: {o['workload']}; yardstick: {o['yardstick']}.  {o['contexts_a_build']} contexts a build, every leg in turn, "
          f"host clock around the call and the synchronise, median of {len(next(iter(L.values()))['runs_ms'])} a leg after a warm-up "
          f"(the fused kernel runs at one of two speeds that stays with a leg and shows in both builds, so the gated ratio is "
          f"the fastest on leg over the fastest yardstick leg):", "",
          "| leg | median ms | min .. max |", "|---|---|---|"]
    md += [f"| {n} | {v['median_ms']} | {v['min_ms']} .. {v['max_ms']} |" for n, v in L.items()]
    md += ["", f"  fastest on {o['on_fastest_ms']} ms over fastest yardstick {o['yardstick_fastest_ms']} ms: ratio "
           f"{o['ratio_on_over_yardstick']} (gate {o['gate']}: {'met' if o['gate_ok'] else 'EXCEEDED'}).  Means over the contexts: on "
           f"{o['on_ms']} ms, this build off {o['this_build_off_ms']} ms, yardstick {o['yardstick_ms']} ms (ratio {o['ratio_of_means']}); "
           f"on / off on the same context, mean {o['ratio_on_over_off_same_context']}.",
           f"- The kernel alone: {k['what']}: median {k['median_ms']} ms ({k['min_ms']} .. {k['max_ms']}), "
           f"{k['GB_per_s']} GB/s of its 6 B a frame, {k['Tops_per_s']} T rounded operations a second."]
    if "stereo" in res:
        s = res["stereo"]
        md.append(f"- Stereo: {s['workload']}; on {s['legs']['on_75us']['median_ms']} ms against {s['legs']['yardstick']['median_ms']} ms "
                  f"({s['yardstick']}), ratio {s['ratio_on_over_yardstick']}, {len(s['legs']['on_75us']['runs_ms'])} runs each.")
    if "bench_py" in res and "parent_median" in res["bench_py"]:
        b = res["bench_py"]
        md.append(f"- Off path (the runs that wrote --ab-dir): `bench.py --gpus 1`, the parent's build and this one alternating, {len(b['parent'])} runs each: parent "
                  f"median {b['parent_median']} MS/s (min {b['parent_min']}, max {b['parent_max']}), this build median {b['this_median']}: "
                  f"{'within' if b['this_median_within_parent_min_max'] else 'OUTSIDE'} the parent's min-to-max spread.")
    md.append("- Not measured: modes 1 to 3, 50 us (the same kernel with other taps), the host-buffer entry points, the tuned and wide "
              "front ends with the stage on, hardware counters (no --pmc run was taken).")
    with open(os.path.join(args.out, "bench_deemph.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
