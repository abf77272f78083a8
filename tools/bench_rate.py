#!/usr/bin/env python3
"""Cost of captures at a rational rate (fmrx_set_capture_rate / fmrx_process_wide_device) on one GPU.

  yardstick: device time of the integer down-converter's launches (csrc/wide.hip) at D = 4, u8, for 1 and
      for 16 stations, over one device-resident capture of 2^29 pairs (1 GiB as u8), mode 0;
  rate: the same for the rational down-converter (csrc/rate.hip) on the same bytes read as a capture at
      10 MS/s (6/25) and at 12.5 MS/s (24/125), u8 and float32 (the same pairs, 4 GiB), 1 and 16 stations.

A leg's time is the sum of the HIP event pairs around its launches on the context stream
(fmrx_kernel_timing), over the whole granules that fit the capture.  Every figure is the median of --reps
runs after a warm-up run, the legs alternating in one loop whose order rotates from run to run.  Per wide
pair the operation count is the integer kernel's (16 taps and one rotation), so the expected ratio of a
leg's time per wide pair and station to the yardstick's at the same station count is about 1.0; the gate
is 1.4.  Writes profiles/rate/bench_rate.json (--out) and a Markdown summary beside it.  No hardware
counters are taken."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

PAIRS = 1 << 29
GATE, EXPECTED = 1.4, 1.0
RF_FS = 2400000


def offsets(n, cap_fs):
    """n offsets on the 100 kHz raster spread over the capture, none of them 0."""
    half = cap_fs // 2 - 200000
    return [100000 * round((-half + (2 * half) * (s + 0.5) / n) / 100000) or 100000 for s in range(n)]


class Leg:
    """The down-converter's launches of one process_wide_device call over the capture."""

    def __init__(self, fm, torch, iq, fmt, cap_fs, stations):
        self.rx = rx = fm.Receiver(0, fm.MONO, rf_taps=101, n_streams=stations)
        if fmt:
            rx.set_input_format(fmt)
        rx.set_capture_rate(cap_fs)
        rx.tune_wide(offsets(stations, cap_fs))
        blocks, pairs = rx.wide_granule
        self.iq, self.ms = iq, []
        self.blocks = PAIRS // pairs * blocks
        self.wide_pairs = PAIRS // pairs * pairs
        self.stations = stations
        self.pcm = torch.empty((stations, self.blocks * rx.geo.pcm_samples), dtype=torch.int16, device="cuda")

    def run(self, keep):
        self.rx.reset()
        self.rx.kernel_timing(1)
        self.rx.process_wide_device(self.iq.data_ptr(), self.blocks, self.pcm.data_ptr())
        self.rx.synchronize()
        avg, launches = self.rx.kernel_timing(-1)
        if keep:
            self.ms.append(avg * launches)

    def summary(self):
        med = statistics.median(self.ms)
        return {"ms_median": med, "ms_min": min(self.ms), "ms_max": max(self.ms), "wide_pairs": self.wide_pairs,
                "stations": self.stations, "ns_per_wide_pair_station": 1e6 * med / self.wide_pairs / self.stations,
                "ms": [round(v, 4) for v in self.ms]}


def alternate(legs, reps):
    order = list(legs.values())
    for r in range(reps + 1):  # the order rotates, so no leg always follows the same neighbour
        for leg in order[r % len(order):] + order[: r % len(order)]:
            leg.run(keep=r > 0)
    out = {k: leg.summary() for k, leg in legs.items()}
    for leg in legs.values():
        leg.rx.close()
    return out


def report(res):
    lines = ["## Rational capture rates: cost of the down-converter (tools/bench_rate.py)", "",
             f"Mode 0, 101 taps, one device-resident capture of 2^29 pairs, median of {res['reps']} runs after a warm-up, "
             f"legs alternating in one loop.  Device: {res['device']}.", "",
             "| leg | ms (min .. max) | ps a wide pair and station | over the D = 4 leg |", "|---|---|---|---|"]
    for k, v in res["legs"].items():
        ratio = res["ratios"].get(k)
        lines.append(f"| {k} | {v['ms_median']:.3f} ({v['ms_min']:.3f} .. {v['ms_max']:.3f}) | "
                     f"{1e3 * v['ns_per_wide_pair_station']:.3f} | " + (f"{ratio:.2f}" if ratio else "yardstick") + " |")
    missed = [k for k, r in res["ratios"].items() if r > GATE]
    lines += ["", f"Expected about {EXPECTED}, gate {GATE}: " +
              ("every leg within the gate." if not missed else "ABOVE the gate: " + ", ".join(missed) + ".")]
    lines.append("Not measured: hardware counters (none were taken), modes 1-3, 51 taps, other ratios, int8 and int16, "
                 "stereo contexts, host-buffer calls, the CLI.")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rate", "bench_rate.json"))
    args = ap.parse_args()
    import torch

    import iqgen

    fm = iqgen.load_fmrx()
    res = {"tool": "tools/bench_rate.py", "mode": 0, "rf_taps": 101, "pairs": PAIRS, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "gate": GATE, "expected": EXPECTED, "hardware_counters": "none taken"}
    with fm.Receiver(0, fm.MONO) as rx:
        u8 = torch.empty(2 * PAIRS, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rx.synth_device(3, 0, PAIRS, u8.data_ptr())
        rx.synchronize()
    f32 = ((u8.to(torch.float32) - 128.0) / 128.0).contiguous()
    legs = {}
    for n in (1, 16):
        legs[f"wide_u8_D4_x{n}"] = Leg(fm, torch, u8, 0, 4 * RF_FS, n)
    for name, cap_fs in (("6_25", 10000000), ("24_125", 12500000)):
        for fmt_name, fmt, iq in (("u8", 0, u8), ("f32", 3, f32)):
            for n in (1, 16):
                legs[f"rate_{fmt_name}_{name}_x{n}"] = Leg(fm, torch, iq, fmt, cap_fs, n)
    torch.cuda.synchronize()
    res["legs"] = alternate(legs, args.reps)
    res["ratios"] = {k: v["ns_per_wide_pair_station"] / res["legs"][f"wide_u8_D4_x{v['stations']}"]["ns_per_wide_pair_station"]
                     for k, v in res["legs"].items() if k.startswith("rate_")}
    res["within_gate"] = all(r <= GATE for r in res["ratios"].values())
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
