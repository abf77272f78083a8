#!/usr/bin/env python3
"""Cost of off-centre tuning (csrc/tuner.hip) on one GPU: mode 0, 101-tap RF, device-resident bytes.

  (a) stage-0 device time (fmrx_debug_stage_timing, "RF front end") of the UNTUNED RF-only front
      end on a stereo context, 16 streams x 64 blocks (serial engine: one front-end launch a call);
  (b) the same bytes with 16 non-zero offsets (the tuned front end, same stage kind);
  (c) a shared capture decoded by 11 mono streams, -1.0 .. +1.0 MHz in 200 kHz steps: wall time
      and IQ MS/s per station.

(a) is the baseline and uses only calls older than the tuner, so it can be taken from a build of
the parent commit: `--legs a --pkg <that build's package dir> --out a_parent.json`, then
`--baseline a_parent.json` on the new build.  Writes profiles/tuner/bench_tuner.json (--out) and
the DESIGN_LOG entry beside it (.md; --log appends it to DESIGN_LOG.md).  HBM bytes per station
need a counter pass of their own (rocprofv3 --pmc, nothing else traced): not taken here."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

STREAMS, BLOCKS, TAPS = 16, 64, 101
OFFSETS_B = [100000 * (s - 8) + (100000 if s >= 8 else 0) for s in range(16)]  # -800 .. +800 kHz, no 0
OFFSETS_C = [200000 * s for s in range(-5, 6)]
LIMIT = 1.3


def load_fmrx(pkg):
    if not pkg:
        import iqgen

        return iqgen.load_fmrx()
    spec = importlib.util.spec_from_file_location("fmrx_pkg", os.path.join(pkg, "fmrx.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def front_end_ms(fm, torch, offsets, reps):
    """Stage-0 device ms of one call, per repetition (the first call warms up and is dropped)."""
    rx = fm.Receiver(0, fm.STEREO, rf_taps=TAPS, n_streams=STREAMS, knobs={"stereo_chunks": 1})
    bb = rx.geo.block_bytes
    iq = torch.empty((STREAMS, BLOCKS * bb), dtype=torch.uint8, device="cuda")
    pcm = torch.empty((STREAMS, BLOCKS * rx.geo.pcm_samples), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rx.synth_device_streams(list(range(STREAMS)), 0, BLOCKS * bb // 2, iq.data_ptr(), BLOCKS * bb)
    if offsets is not None:
        rx.tune(offsets)
    out = []
    for r in range(reps + 1):
        rx.reset()
        rx.stage_timing(1)
        rx.process_device(iq.data_ptr(), BLOCKS, pcm.data_ptr())
        rx.synchronize()
        ms, launches, _ = rx.stage_timing(-1)["front_end"]
        assert launches == 1, launches
        if r:
            out.append(ms)
    rx.close()
    return out


def shared_capture(fm, torch, blocks, reps):
    ns = len(OFFSETS_C)
    rx = fm.Receiver(0, fm.MONO, rf_taps=TAPS, n_streams=ns)
    bb = rx.geo.block_bytes
    iq = torch.empty(blocks * bb, dtype=torch.uint8, device="cuda")
    pcm = torch.empty((ns, blocks * rx.geo.pcm_samples), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rx.synth_device(3, 0, blocks * bb // 2, iq.data_ptr())
    rx.tune(OFFSETS_C)
    wall = []
    for r in range(reps + 1):
        rx.reset()
        t0 = time.perf_counter()
        rx.process_shared_device(iq.data_ptr(), blocks, pcm.data_ptr())
        rx.synchronize()
        if r:
            wall.append(time.perf_counter() - t0)
    pairs = blocks * bb // 2
    rx.close()
    dt = statistics.median(wall)
    return {"stations": ns, "offsets_hz": OFFSETS_C, "blocks": blocks, "capture_seconds": pairs / 2.4e6,
            "wall_s_median": dt, "wall_s_min": min(wall), "iq_MS_per_s_per_station": pairs / dt / 1e6,
            "iq_MS_per_s_all_stations": ns * pairs / dt / 1e6, "x_realtime": pairs / 2.4e6 / dt,
            "hbm_bytes_read_per_station": None}


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms": [round(v, 5) for v in ms]}


def entry(res):
    a, b, c = res.get("a"), res.get("b"), res.get("c")
    lines = ["## Off-centre tuning: cost of the tuned front end (tools/bench_tuner.py)", "",
             f"Mode 0, {TAPS}-tap RF, device-resident bytes, {STREAMS} streams x {BLOCKS} blocks "
             "(stereo context, serial engine), stage-0 device time from HIP events, median of "
             f"{res['reps']} calls after a warm-up call."]
    if a:
        lines.append(f"- (a) untuned front end ({res['a_source']}): {a['ms_median']:.4f} ms (min {a['ms_min']:.4f})")
    if b:
        lines.append(f"- (b) tuned front end, 16 non-zero offsets: {b['ms_median']:.4f} ms (min {b['ms_min']:.4f})")
    if a and b:
        ratio = res["ratio_b_over_a"]
        lines.append(f"- (b)/(a) = {ratio:.3f} against the expected <= {LIMIT}: " + ("within it." if ratio <= LIMIT else
                     "ABOVE it -- see the per-chunk instruction accounting below before tuning anything."))
    if c:
        lines.append(f"- (c) shared capture, {c['stations']} mono stations (-1.0 .. +1.0 MHz), {c['blocks']} blocks "
                     f"({c['capture_seconds']:.2f} s of signal): wall {c['wall_s_median'] * 1e3:.2f} ms, "
                     f"{c['iq_MS_per_s_per_station']:.0f} IQ MS/s per station ({c['iq_MS_per_s_all_stations']:.0f} "
                     f"over all stations, {c['x_realtime']:.0f} x real time for the capture).")
    lines.append("- Not measured: HBM bytes read per station (no counter pass was taken), the tuned front end in "
                 "modes 1-3 and with 51 taps, tuned stereo calls end to end, many-stream (> 16) tuned calls.")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--blocks-shared", type=int, default=2048)
    ap.add_argument("--pkg", default=None, help="package directory of another build (leg a of the parent commit)")
    ap.add_argument("--baseline", default=None, help="JSON of a `--legs a` run of the parent commit's build")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tuner", "bench_tuner.json"))
    ap.add_argument("--log", action="store_true", help="append the entry to DESIGN_LOG.md")
    args = ap.parse_args()
    import torch

    fm = load_fmrx(args.pkg)
    res = {"tool": "tools/bench_tuner.py", "mode": 0, "rf_taps": TAPS, "streams": STREAMS, "blocks": BLOCKS,
           "reps": args.reps, "device": torch.cuda.get_device_name(0), "limit_b_over_a": LIMIT}
    if args.baseline:
        with open(args.baseline) as f:
            base = json.load(f)
        res["a"], res["a_source"] = base["a"], "build of the parent commit, same machine and session"
    elif "a" in args.legs:
        res["a"] = summary(front_end_ms(fm, torch, None, args.reps))
        res["a_source"] = "this build's untuned kernel (its sources are the parent commit's)" if not args.pkg else args.pkg
    if "b" in args.legs:
        res["offsets_b_hz"] = OFFSETS_B
        res["b"] = summary(front_end_ms(fm, torch, OFFSETS_B, args.reps))
    if "a" in res and "b" in res:
        res["ratio_b_over_a"] = res["b"]["ms_median"] / res["a"]["ms_median"]
        res["within_limit"] = res["ratio_b_over_a"] <= LIMIT
    if "c" in args.legs:
        res["c"] = shared_capture(fm, torch, args.blocks_shared, max(3, args.reps // 3))
    res["not_measured"] = ["HBM bytes read per station (no counter pass)", "modes 1-3 and 51 taps tuned",
                           "tuned stereo calls end to end", "more than 16 tuned streams"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    text = entry(res)
    with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
        f.write(text)
    if args.log:
        with open(os.path.join(REPO, "DESIGN_LOG.md"), "a") as f:
            f.write("\n" + text)
    print(text)
    print(json.dumps({k: res[k] for k in ("a", "b", "ratio_b_over_a", "c") if k in res}))


if __name__ == "__main__":
    main()
