#!/usr/bin/env python3
"""AFC on one GPU, one run.

    python tools/bench_afc.py [--streams 256] [--seconds 9.984] [--repeats 15] [--ab-dir DIR]
                              [--out profiles/afc]

Four legs.  kernel: fmrx_carrier_device and fmrx_meter_device over the same device-resident mode-0 rows,
alternating, HIP events on the context's stream, bytes read over time against a device-to-device copy of
those rows taken in the same run.  switch: a tuned mono fmrx_process_device call, 16 streams x 3.072 s,
fmrx_set_afc off, on without tracking, and on beside the meter, in turn (wall clock, the call's host
synchronisation included).  retune: what one retune costs, fmrx_tune of all streams at the context's
position on an idle stream (a stream drain and two uploads; wall clock).  --ab-dir: bench.py result lines,
parent_*.json and this_*.json from alternating runs of the parent's and this build.  Writes bench_afc.json
and bench_afc.md under --out; every number in them was measured by this run (the bench.py lines by the runs
that wrote --ab-dir).
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


def kernel(torch, fm, iqgen, ns, seconds, repeats):
    with fm.Receiver(0, fm.MONO, n_streams=ns) as rx:
        g, nif, bp_fs = rx.rds_granule, rx.geo.if_samples, rx.geo.bp_fs
        nb = int(round(seconds * bp_fs)) // (nif * g) * g
        n = nb * nif
        frames = n // (fm.METER_WINDOWS * (bp_fs // 1000))
        row = torch.from_numpy(iqgen.make_rds_demod(3, n, bp_fs)).cuda()
        d_in = row.repeat(ns, 1).contiguous()
        d_pow = torch.empty((ns, frames, fm.METER_TONES), dtype=torch.float32, device="cuda")
        d_sums = torch.empty((ns, frames, 2), dtype=torch.float32, device="cuda")
        stream = torch.cuda.ExternalStream(rx.stream())
        legs = {"carrier": lambda: rx.carrier_device(d_in.data_ptr(), nb, d_sums.data_ptr()),
                "meter": lambda: rx.meter_device(d_in.data_ptr(), nb, d_pow.data_ptr())}
        for run in legs.values():  # warm-up: the code objects, the meter's tables
            run(), rx.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(repeats):
            for k, run in legs.items():
                ms[k].append(round(event_ms(torch, stream, run), 4))
        rep = fm.carrier_accumulate(d_sums[0].cpu().numpy())
        dec = fm.afc_decide(rep, bp_fs)
        hbm = copy_gbs(torch, d_in)
    read = 4.0 * ns * n
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"workload": f"fmrx_carrier_device and fmrx_meter_device alternating, mode 0, {ns} stream(s) x {n / bp_fs:.3f} s of device rows "
                        f"({read / 1e9:.3f} GB read)",
            "carrier_ms": ms["carrier"], "meter_ms": ms["meter"], "carrier_ms_median": med["carrier"], "meter_ms_median": med["meter"],
            "carrier_read_GBs": round(read / (med["carrier"] * 1e-3) / 1e9, 1), "meter_read_GBs": round(read / (med["meter"] * 1e-3) / 1e9, 1),
            "copy_GBs_read_plus_written": hbm, "copy_read_GBs": round(hbm / 2, 1),
            "carrier_over_copy_read_rate": round(read / (med["carrier"] * 1e-3) / 1e9 / (hbm / 2), 3),
            "not_slower_than_meter": bool(med["carrier"] <= med["meter"]),
            "stream0_err_hz": round(dec["err_hz"], 2), "stream0_mean_square": round(dec["mean_square"], 5)}


def switch(torch, fm, iqgen, ns, repeats):
    """A tuned mono process_device call of 48 granules a stream: the switch off, on (measuring only), on beside
    the meter, and the meter alone, in turn."""
    legs = {"off": (False, False), "afc": (True, False), "meter": (False, True), "afc_and_meter": (True, True)}
    with fm.Receiver(0, fm.MONO, n_streams=ns) as rx:
        nb = 48 * rx.rds_granule
        iq = iqgen.make("synth:3", nb * rx.geo.block_bytes, rx.geo.rf_fs)
        d_iq = torch.from_numpy(np.tile(iq, (ns, 1))).cuda()
        d_pcm = torch.empty((ns, nb * rx.geo.pcm_samples), dtype=torch.int16, device="cuda")
        rx.tune([0] * ns)
        out = {k + "_ms": [] for k in legs}
        for r in range(repeats + 1):
            for k, (afc, meter) in legs.items():
                rx.reset()
                rx.set_afc(afc, track=0)
                rx.set_meter(meter)
                t0 = time.perf_counter()
                rx.process_device(d_iq.data_ptr(), nb, d_pcm.data_ptr())
                rx.synchronize()
                if r >= 1:  # the first round sizes the buffers
                    out[k + "_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        sig = nb * rx.geo.if_samples / rx.geo.bp_fs
        # one retune: all streams moved by a step at the context's position, the stream idle
        tune_ms = []
        for r in range(repeats + 1):
            offs, pos, _ = rx.tuner_info()
            rx.synchronize()
            t0 = time.perf_counter()
            rx.tune([1000 * ((r + k) % 7) for k in range(ns)], pos)
            if r >= 1:
                tune_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    for k in legs:
        out[k + "_ms_median"] = statistics.median(out[k + "_ms"])
    out.update(workload=f"tuned fmrx_process_device, mode 0 mono, {ns} stream(s) x {sig:.3f} s, wall clock",
               retune_ms=tune_ms, retune_ms_median=statistics.median(tune_ms),
               retune_workload=f"fmrx_tune of {ns} stream(s) on an idle stream (a drain and two uploads), wall clock")
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
        out.update(parent_median=statistics.median(pv), this_median=statistics.median(tv), parent_min=min(pv), parent_max=max(pv),
                   parent_spread=round(max(pv) - min(pv), 1))
        out["within_parent_spread"] = bool(abs(out["parent_median"] - out["this_median"]) <= out["parent_spread"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=9.984)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--switch-streams", type=int, default=16)
    ap.add_argument("--switch-repeats", type=int, default=5)
    ap.add_argument("--ab-dir")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "afc"))
    args = ap.parse_args()
    import torch

    import iqgen

    fm = iqgen.load_fmrx()
    prop = torch.cuda.get_device_properties(0)
    arch = getattr(prop, "gcnArchName", "?").split(":")[0]
    # the runtime names the card generically; gfx950 with 256 CUs is the MI355X
    card = "MI355X" if arch == "gfx950" and prop.multi_processor_count == 256 else "GPU"
    res = {"gpu": f"{card} ({torch.cuda.get_device_name(0)}, {arch}, {prop.multi_processor_count} CUs)", "measured_on_gpu": True,
           "kernel": kernel(torch, fm, iqgen, args.streams, args.seconds, args.repeats),
           "switch": switch(torch, fm, iqgen, args.switch_streams, args.switch_repeats)}
    if args.ab_dir:
        res["bench_py"] = bench_ab(args.ab_dir)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_afc.json"), "w") as f:
        json.dump(res, f, indent=1)
    k, s = res["kernel"], res["switch"]
    md = ["## AFC (bench_afc.json)", "",
          f"Every number below was measured on one {res['gpu']} by one run of `tools/bench_afc.py`; nothing here is an "
          f"estimate or a CPU figure.", "",
          f"- {k['workload']}, HIP events, {len(k['carrier_ms'])} repeats each after a warm-up: the carrier sums median "
          f"{k['carrier_ms_median']} ms = {k['carrier_read_GBs']} GB/s read ({k['carrier_ms']}); the meter kernel median "
          f"{k['meter_ms_median']} ms = {k['meter_read_GBs']} GB/s ({k['meter_ms']}).  A device-to-device copy of the same rows "
          f"moves {k['copy_GBs_read_plus_written']} GB/s read + written, {k['copy_read_GBs']} GB/s each way: the carrier sums "
          f"read at {k['carrier_over_copy_read_rate']} of the copy's read rate.",
          f"- {s['workload']}, in turn: off median {s['off_ms_median']} ms, `fmrx_set_afc` (track 0) {s['afc_ms_median']} ms, "
          f"`fmrx_set_meter` {s['meter_ms_median']} ms, both {s['afc_and_meter_ms_median']} ms (off {s['off_ms']}, afc {s['afc_ms']}, "
          f"meter {s['meter_ms']}, both {s['afc_and_meter_ms']}).",
          f"- {s['retune_workload']}: median {s['retune_ms_median']} ms ({s['retune_ms']})."]
    if "bench_py" in res and "parent_median" in res["bench_py"]:
        b = res["bench_py"]
        md.append(f"- `bench.py --gpus 1 --steps 20 --warmup 3`, the parent's build and this one alternating, {len(b['parent'])} runs "
                  f"each: parent median {b['parent_median']} MS/s (min {b['parent_min']}, max {b['parent_max']}), this build "
                  f"{b['this_median']} MS/s: {'within' if b['within_parent_spread'] else 'OUTSIDE'} the parent's min-to-max spread.  "
                  f"The headline path (untuned mono) never reaches the switch, which is off by default.")
    md.append("- Not measured: modes 1 to 3, the host-buffer form, hardware counters, an off-air capture.")
    with open(os.path.join(args.out, "bench_afc.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
