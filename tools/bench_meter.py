#!/usr/bin/env python3
"""The subcarrier meter on one GPU, one run.

    python tools/bench_meter.py [--streams 256] [--seconds 9.984] [--repeats 5] [--ab-dir DIR]
                                [--out profiles/meter]

Four legs.  kernel: fmrx_meter_device over device-resident mode-0 rows, HIP events on the context's
stream, bytes read over time against a device-to-device copy of the same rows (bench.py's
hbm_attainable_GBs, taken here on the same box).  switch: a tuned mono fmrx_process_device call, 16 streams x
3.072 s, fmrx_set_meter off and on alternating (wall clock, the call's host synchronisation included).
payoff: decode_stations(channels=STEREO, rds=True) on an 8-station capture of about 2 s of which four carry
no pilot and four no RDS, probe=False against probe=True (wall clock).  --ab-dir: bench.py result lines,
parent_*.json and this_*.json from alternating runs of the parent's and this build.  Writes
bench_meter.json and bench_meter.md under --out; every number in them was measured by this run (the
bench.py lines by the runs that wrote --ab-dir).
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
        stream = torch.cuda.ExternalStream(rx.stream())
        run = lambda: rx.meter_device(d_in.data_ptr(), nb, d_pow.data_ptr())
        run(), rx.synchronize()  # warm-up: the code object, the tables
        ms = [round(event_ms(torch, stream, run), 4) for _ in range(repeats)]
        lv = fm.meter_detect(fm.meter_accumulate(d_pow[0].cpu().numpy()))
        hbm = copy_gbs(torch, d_in)
    med = statistics.median(ms)
    read = 4.0 * ns * n
    return {"workload": f"fmrx_meter_device, mode 0, {ns} stream(s) x {n / bp_fs:.3f} s of device rows ({read / 1e9:.3f} GB read)",
            "ms": ms, "ms_median": med, "read_GBs": round(read / (med * 1e-3) / 1e9, 1), "hbm_attainable_GBs": hbm,
            "fraction_of_attainable": round(read / (med * 1e-3) / 1e9 / hbm, 3),
            "rounded_ops_per_s_T": round(28.0 * ns * n / (med * 1e-3) / 1e12, 2),
            "stream0_pilot_snr_db": round(lv["pilot_snr_db"], 2), "stream0_rds_snr_db": round(lv["rds_snr_db"], 2)}


def switch(torch, fm, iqgen, ns, repeats):
    """A tuned mono process_device call of 48 granules a stream, fmrx_set_meter off and on, alternating."""
    with fm.Receiver(0, fm.MONO, n_streams=ns) as rx:
        nb = 48 * rx.rds_granule
        iq = iqgen.make("synth:3", nb * rx.geo.block_bytes, rx.geo.rf_fs)
        d_iq = torch.from_numpy(np.tile(iq, (ns, 1))).cuda()
        d_pcm = torch.empty((ns, nb * rx.geo.pcm_samples), dtype=torch.int16, device="cuda")
        rx.tune([0] * ns)
        out = {"off_ms": [], "on_ms": []}
        for k in range(2 * (repeats + 1)):
            on = k % 2 == 1
            rx.reset()
            rx.set_meter(on)
            t0 = time.perf_counter()
            rx.process_device(d_iq.data_ptr(), nb, d_pcm.data_ptr())
            rx.synchronize()
            if k >= 2:  # the first pair sizes the buffers
                out["on_ms" if on else "off_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        sig = nb * rx.geo.if_samples / rx.geo.bp_fs
    out.update(workload=f"tuned fmrx_process_device, mode 0 mono, {ns} stream(s) x {sig:.3f} s, wall clock",
               off_ms_median=statistics.median(out["off_ms"]), on_ms_median=statistics.median(out["on_ms"]))
    return out


def station(iqgen, n, offset_hz, seed, audio_hz, pilot, lr, rds, rf_fs=2400000, rf_decim=10):
    """One FM station as unit-amplitude complex samples: a mono tone, optionally the pilot with an L-R tone
    pair around 38 kHz, optionally biphase symbols of random bits at 1187.5 bit/s on 57 kHz (no groups: the
    decoder's work does not depend on what the bits say).  The phase is the running sum of the multiplex."""
    t = np.arange(n, dtype=np.float64) / rf_fs
    m = 0.30 * np.sin(2 * np.pi * audio_hz * t)
    if pilot:
        m += pilot * np.cos(2 * np.pi * 19000.0 * t) + lr * np.sin(2 * np.pi * 700.0 * t) * np.cos(2 * np.pi * 38000.0 * t)
    if rds:
        ph = t * 1187.5
        k = np.floor(ph).astype(np.int64)
        sym = 2.0 * (iqgen.rand_bytes(seed + 40, int(k[-1]) + 1) & 1).astype(np.float64) - 1.0
        m += rds * sym[k] * np.where(ph - k < 0.5, 1.0, -1.0) * np.cos(2 * np.pi * 57000.0 * t)
    return np.exp(1j * (np.cumsum(m / rf_decim) + 2 * np.pi * offset_hz * t))


def payoff(fm, iqgen, repeats, frames=32):
    """Eight stations 250 kHz apart, about 2 s: pilot and RDS, pilot alone, RDS alone, neither, twice over."""
    kinds = [dict(pilot=0.05, lr=0.1, rds=0.04), dict(pilot=0.05, lr=0.1, rds=0.0), dict(pilot=0.0, lr=0.0, rds=0.04),
             dict(pilot=0.0, lr=0.0, rds=0.0)] * 2
    offs = [-900000 + 250000 * k for k in range(8)]
    n = frames * 24 * 6400
    z = sum(station(iqgen, n, o, k + 1, 500.0 * (k + 1), **kw) for k, (o, kw) in enumerate(zip(offs, kinds)))
    raw = np.empty(2 * n)
    raw[0::2], raw[1::2] = 128.0 + 14.0 * z.real, 128.0 + 14.0 * z.imag
    dither = (iqgen.rand_bytes(99, 2 * n).astype(np.float64) - 127.5) / 127.5  # +-1 LSB: a receiver's noise floor
    iq = np.clip(np.round(raw + dither), 0, 255).astype(np.uint8)
    out = {"plain_ms": [], "probe_ms": []}
    res = {}
    for k in range(2 * (repeats + 1)):
        probe = k % 2 == 1
        t0 = time.perf_counter()
        r = fm.decode_stations(iq, channels=fm.STEREO, rds=True, probe=probe)
        if k >= 2:
            out["probe_ms" if probe else "plain_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
        res[probe] = r
    found = [s.offset_hz for s in res[True][0]]
    flags = [(lv["stereo"], lv["rds"]) for lv in res[True][3]]
    named = [None if i is None else i["groups"] for i in res[True][2]]
    for key in ("plain_ms", "probe_ms"):
        out[key + "_median"] = statistics.median(out[key])
        out[key + "_min_max"] = [min(out[key]), max(out[key])]
    out.update(workload=f"decode_stations(channels=STEREO, rds=True), mode 0, 8 stations x {frames * 0.064:.3f} s of u8, wall clock "
                        f"(scan, contexts and host copies included)",
               stations_found=found, expected_flags=[(int(bool(kw["pilot"])), int(bool(kw["rds"]))) for kw in kinds],
               flags=flags, groups=named, groups_plain=[i["groups"] for i in res[False][2]])
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
        out["within_parent_spread"] = bool(out["parent_median"] - out["this_median"] <= out["parent_spread"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=9.984)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--switch-streams", type=int, default=16)
    ap.add_argument("--ab-dir")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "meter"))
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
           "switch": switch(torch, fm, iqgen, args.switch_streams, args.repeats),
           "payoff": payoff(fm, iqgen, args.repeats)}
    if args.ab_dir:
        res["bench_py"] = bench_ab(args.ab_dir)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_meter.json"), "w") as f:
        json.dump(res, f, indent=1)
    k, s, p = res["kernel"], res["switch"], res["payoff"]
    md = ["## The subcarrier meter (bench_meter.json)", "",
          f"Every number below was measured on one {res['gpu']} by one run of `tools/bench_meter.py`; nothing here is an "
          f"estimate or a CPU figure.", "",
          f"- {k['workload']}, HIP events, {len(k['ms'])} repeats after a warm-up: {k['ms']} ms, median {k['ms_median']} ms = "
          f"{k['read_GBs']} GB/s read, {k['rounded_ops_per_s_T']} T rounded operations a second.  A device-to-device copy of "
          f"the same rows moves {k['hbm_attainable_GBs']} GB/s (read + written): the meter reaches "
          f"{k['fraction_of_attainable']} of it.",
          f"- {s['workload']}, `fmrx_set_meter` off and on alternating: median {s['off_ms_median']} ms off, "
          f"{s['on_ms_median']} ms on (off {s['off_ms']}, on {s['on_ms']}).",
          f"- {p['workload']}: probe=False median {p['plain_ms_median']} ms (min, max {p['plain_ms_min_max']}), probe=True median "
          f"{p['probe_ms_median']} ms ({p['probe_ms_min_max']}).  Stations found at {p['stations_found']}; flags (stereo, rds) "
          f"{p['flags']} against {p['expected_flags']} built in; groups with probe {p['groups']}, without {p['groups_plain']}."]
    if "bench_py" in res and "parent_median" in res["bench_py"]:
        b = res["bench_py"]
        md.append(f"- `bench.py --gpus 1 --steps 20 --warmup 3`, the parent's build and this one alternating, {len(b['parent'])} runs "
                  f"each: parent median {b['parent_median']} MS/s (min {b['parent_min']}, max {b['parent_max']}), this build "
                  f"{b['this_median']} MS/s: {'within' if b['within_parent_spread'] else 'OUTSIDE'} the parent's min-to-max spread.  "
                  f"The headline path (untuned mono) never reaches the meter; the switch is off by default.")
    md.append("- Not measured: modes 1 to 3, the host-buffer form, hardware counters.")
    with open(os.path.join(args.out, "bench_meter.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
