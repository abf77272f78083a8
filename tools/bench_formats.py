#!/usr/bin/env python3
"""Cost of the raw I/Q formats (fmrx_set_input_format: u8, s8, s16, f32) on one GPU.

  front end: stage-0 device time (fmrx_debug_stage_timing, "RF front end") of the tuned front end
      (csrc/tuner.hip), mode 0, 101-tap RF, 16 streams x 512 blocks at 16 non-zero offsets (stereo
      context, serial engine: one front-end launch a call), the same pairs in all four formats --
      one synth capture, identity-mapped on the device (u ^ 0x80, (u - 128) * 256, (u - 128) / 128);
  scan: device time (events on the context stream) of fmrx_scan_spectrum_device at 4096 bins over
      2^29 pairs (1 GiB as u8; 1, 2 and 4 GiB as s8, s16 and f32), the same pairs again.

Every figure is the median of --reps runs after a warm-up run, the legs alternating in one loop
whose order rotates from run to run.
The baseline is the PARENT commit's tuned u8 front end, from a build of that commit in another
directory (--parent-pkg: its package directory) loaded beside this one and timed in the same loop;
its own spread (max - min over its runs) is the noise the u8 leg is judged against.  Writes
profiles/formats/bench_formats.json (--out) and a Markdown summary beside it.  No hardware
counters are taken."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

STREAMS, BLOCKS, TAPS = 16, 512, 101  # 52 M pairs a call: the front end runs for ~0.1 ms
OFFSETS = [100000 * (s - 8) + (100000 if s >= 8 else 0) for s in range(16)]  # -800 .. +800 kHz, no 0
SCAN_PAIRS, SCAN_BINS = 1 << 29, 4096
NAMES = ["u8", "s8", "s16", "f32"]
EXPECTED = {"u8": "within the parent's run-to-run spread", "s8": "the same as u8", "s16": "at most about 1.1x",
            "f32": "bounded by its 4x input bytes, not by conversion"}


def load_fmrx(pkg):
    if not pkg:
        import iqgen

        return iqgen.load_fmrx()
    spec = importlib.util.spec_from_file_location("fmrx_parent", os.path.join(pkg, "fmrx.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def mapped(torch, u8, fmt):
    """The u8 tensor's pairs in another format, the normalised samples unchanged."""
    if fmt == 0:
        return u8
    if fmt == 1:
        return (u8 ^ 0x80).view(torch.int8)
    if fmt == 2:
        return (u8.to(torch.int16) - 128) * 256
    return (u8.to(torch.float32) - 128.0) / 128.0


class FrontLeg:
    def __init__(self, fm, torch, u8, fmt):
        self.rx = fm.Receiver(0, fm.STEREO, rf_taps=TAPS, n_streams=STREAMS, knobs={"stereo_chunks": 1})
        if fmt:
            self.rx.set_input_format(fmt)
        self.iq = mapped(torch, u8, fmt).contiguous()
        self.pcm = torch.empty((STREAMS, BLOCKS * self.rx.geo.pcm_samples), dtype=torch.int16, device="cuda")
        self.rx.tune(OFFSETS)
        self.ms = []

    def run(self, keep):
        self.rx.reset()
        self.rx.stage_timing(1)
        self.rx.process_device(self.iq.data_ptr(), BLOCKS, self.pcm.data_ptr())
        self.rx.synchronize()
        ms, launches, _ = self.rx.stage_timing(-1)["front_end"]
        assert launches == 1, launches
        if keep:
            self.ms.append(ms)


class ScanLeg:
    def __init__(self, fm, torch, u8, fmt):
        self.torch = torch
        self.rx = fm.Receiver(0, fm.MONO)
        if fmt:
            self.rx.set_input_format(fmt)
        self.iq = mapped(torch, u8, fmt).contiguous()
        self.power = torch.empty(SCAN_BINS, dtype=torch.float32, device="cuda")
        self.stream = torch.cuda.ExternalStream(self.rx.stream())
        self.ms = []

    def run(self, keep):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        self.rx.scan_spectrum_device(self.iq.data_ptr(), SCAN_PAIRS, SCAN_BINS, self.power.data_ptr())
        e1.record(self.stream)
        self.rx.synchronize()
        e1.synchronize()
        if keep:
            self.ms.append(e0.elapsed_time(e1))


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_spread": max(ms) - min(ms),
            "ms": [round(v, 5) for v in ms]}


def alternate(legs, reps):
    order = list(legs.values())
    for r in range(reps + 1):  # the order rotates, so no leg always follows the same neighbour
        for leg in order[r % len(order):] + order[: r % len(order)]:
            leg.run(keep=r > 0)
    out = {k: summary(leg.ms) for k, leg in legs.items()}
    for leg in legs.values():
        leg.rx.close()
    return out


def report(res):
    lines = ["## Raw I/Q formats: cost of the tuned front end and of the scan (tools/bench_formats.py)", "",
             f"Mode 0, {TAPS}-tap RF, {STREAMS} streams x {BLOCKS} blocks at 16 non-zero offsets, device-resident, the same "
             f"pairs in every format; stage-0 device time, median of {res['reps']} runs after a warm-up, legs alternating "
             f"in one loop.  Device: {res['device']}."]
    base = res["front_end"].get("parent_u8")
    if base:
        lines.append(f"- parent commit, tuned u8: {base['ms_median']:.4f} ms (min {base['ms_min']:.4f}, max {base['ms_max']:.4f}: "
                     f"spread {base['ms_spread']:.4f} ms)")
    for k in NAMES:
        v = res["front_end"][k]
        rel = f", {v['ms_median'] / base['ms_median']:.3f}x the parent's u8" if base else ""
        lines.append(f"- {k}: {v['ms_median']:.4f} ms (min {v['ms_min']:.4f}, max {v['ms_max']:.4f}){rel}; expected: {EXPECTED[k]}")
    if "u8_regression" in res:
        lines.append(f"- u8 against the parent: median difference {res['u8_minus_parent_ms']:+.4f} ms, the parent's own spread "
                     f"{base['ms_spread']:.4f} ms: " + ("a regression beyond the spread." if res["u8_regression"] else
                                                         "no regression beyond the spread."))
    if res.get("scan"):
        lines.append(f"- scan, {SCAN_BINS} bins over 2^29 pairs (device time between events on the context stream):")
        for k in NAMES:
            v = res["scan"][k]
            gib = SCAN_PAIRS * res["pair_bytes"][k] / 2 ** 30
            lines.append(f"  - {k}: {v['ms_median']:.3f} ms (min {v['ms_min']:.3f}, max {v['ms_max']:.3f}), {gib:.0f} GiB read: "
                         f"{gib * 2 ** 30 / v['ms_median'] / 1e9:.2f} TB/s")
    lines.append("- Not measured: hardware counters (none were taken), modes 1-3 and 51 taps, host-buffer calls, the CLI.")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--parent-pkg", default=None, help="package directory of a build of the parent commit")
    ap.add_argument("--no-scan", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "formats", "bench_formats.json"))
    args = ap.parse_args()
    import torch

    fm = load_fmrx(None)
    res = {"tool": "tools/bench_formats.py", "mode": 0, "rf_taps": TAPS, "streams": STREAMS, "blocks": BLOCKS,
           "offsets_hz": OFFSETS, "reps": args.reps, "device": torch.cuda.get_device_name(0), "expected": EXPECTED,
           "pair_bytes": {k: fm.iq_pair_bytes(i) for i, k in enumerate(NAMES)},
           "hardware_counters": "none taken"}
    with fm.Receiver(0, fm.MONO) as rx:
        bb = rx.geo.block_bytes
        u8 = torch.empty((STREAMS, BLOCKS * bb), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rx.synth_device_streams(list(range(STREAMS)), 0, BLOCKS * bb // 2, u8.data_ptr(), BLOCKS * bb)
        rx.synchronize()
    legs = {}
    if args.parent_pkg:
        legs["parent_u8"] = FrontLeg(load_fmrx(args.parent_pkg), torch, u8, 0)
    for i, k in enumerate(NAMES):
        legs[k] = FrontLeg(fm, torch, u8, i)
    torch.cuda.synchronize()
    res["front_end"] = alternate(legs, args.reps)
    if args.parent_pkg:
        base, new = res["front_end"]["parent_u8"], res["front_end"]["u8"]
        res["baseline"] = "build of the parent commit, same machine, same process, same loop"
        res["u8_minus_parent_ms"] = new["ms_median"] - base["ms_median"]
        res["u8_regression"] = res["u8_minus_parent_ms"] > base["ms_spread"]
        res["ratio_to_parent_u8"] = {k: res["front_end"][k]["ms_median"] / base["ms_median"] for k in NAMES}
    del legs, u8
    if not args.no_scan:
        with fm.Receiver(0, fm.MONO) as rx:
            u8 = torch.empty(2 * SCAN_PAIRS, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rx.synth_device(3, 0, SCAN_PAIRS, u8.data_ptr())
            rx.synchronize()
        legs = {k: ScanLeg(fm, torch, u8, i) for i, k in enumerate(NAMES)}
        torch.cuda.synchronize()
        res["scan"] = alternate(legs, args.reps)
        res["scan_pairs"], res["scan_bins"] = SCAN_PAIRS, SCAN_BINS
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    text = report(res)
    with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
