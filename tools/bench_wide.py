#!/usr/bin/env python3
"""Cost of wide captures (fmrx_set_capture_decim / fmrx_process_wide_device) on one GPU.

  ddc: device time of the down-converter's launches alone (csrc/wide.hip; HIP event pairs around each
      launch on the context stream, summed over the call's internal pieces: fmrx_kernel_timing) over one
      device-resident capture of 2^29 pairs (1 GiB as u8), mode 0: u8 at D = 4 and D = 8 for 1 and for
      16 stations, int16 and float32 (the same pairs, 2 and 4 GiB) at D = 4;
  call: the whole fmrx_process_wide_device call for 16 mono stations at D = 4, u8 (events around it);
  mono: the yardstick -- the existing 101-tap mode-0 fmrx_process_device call on the same GiB read as one
      narrow stream, in the same loop.

Every figure is the median of --reps runs after a warm-up run, the legs alternating in one loop whose
order rotates from run to run.  The gate: the down-converter's time per station (16 stations, D = 4,
u8) over the mono call's time is at most 2.5 (about 70 separately rounded f32 operations a wide pair
against the fused kernel's 40: 1.8 expected).  Writes profiles/wide/bench_wide.json (--out) and a
Markdown summary beside it.  No hardware counters are taken."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

PAIRS = 1 << 29
GATE, EXPECTED = 2.5, 1.8
RF_FS = 2400000


def offsets(n, d):
    """n offsets on the 100 kHz raster spread over the capture, none of them 0."""
    half = d * RF_FS // 2 - 200000
    return [100000 * round((-half + (2 * half) * (s + 0.5) / n) / 100000) or 100000 for s in range(n)]


def mapped(torch, u8, fmt):
    if fmt == 0:
        return u8
    if fmt == 2:
        return (u8.to(torch.int16) - 128) * 256
    return (u8.to(torch.float32) - 128.0) / 128.0


class Leg:
    def __init__(self, torch, rx):
        self.torch, self.rx, self.ms = torch, rx, []
        self.stream = torch.cuda.ExternalStream(rx.stream())

    def timed(self, fn):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        fn()
        e1.record(self.stream)
        self.rx.synchronize()
        e1.synchronize()
        return e0.elapsed_time(e1)


class WideLeg(Leg):
    """what = "ddc": the down-converter's launches alone; "call": the whole call."""

    def __init__(self, fm, torch, iq, fmt, d, stations, what):
        rx = fm.Receiver(0, fm.MONO, rf_taps=101, n_streams=stations)
        if fmt:
            rx.set_input_format(fmt)
        rx.set_capture_decim(d)
        rx.tune_wide(offsets(stations, d))
        super().__init__(torch, rx)
        self.iq, self.what = iq, what
        self.blocks = PAIRS // (d * rx.geo.iq_pairs)
        self.pcm = torch.empty((stations, self.blocks * rx.geo.pcm_samples), dtype=torch.int16, device="cuda")

    def run(self, keep):
        self.rx.reset()
        if self.what == "ddc":
            self.rx.kernel_timing(1)
        ms = self.timed(lambda: self.rx.process_wide_device(self.iq.data_ptr(), self.blocks, self.pcm.data_ptr()))
        if self.what == "ddc":
            avg, launches = self.rx.kernel_timing(-1)
            ms = avg * launches
        if keep:
            self.ms.append(ms)


class MonoLeg(Leg):
    def __init__(self, fm, torch, iq):
        super().__init__(torch, fm.Receiver(0, fm.MONO, rf_taps=101))
        self.iq = iq
        self.blocks = PAIRS // self.rx.geo.iq_pairs
        self.pcm = torch.empty(self.blocks * self.rx.geo.pcm_samples, dtype=torch.int16, device="cuda")

    def run(self, keep):
        self.rx.reset()
        ms = self.timed(lambda: self.rx.process_device(self.iq.data_ptr(), self.blocks, self.pcm.data_ptr()))
        if keep:
            self.ms.append(ms)


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms": [round(v, 4) for v in ms]}


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
    lines = ["## Wide captures: cost of the down-converter (tools/bench_wide.py)", "",
             f"Mode 0, one device-resident capture of 2^29 pairs, median of {res['reps']} runs after a warm-up, legs "
             f"alternating in one loop.  Device: {res['device']}."]
    for k, v in res["legs"].items():
        lines.append(f"- {k}: {v['ms_median']:.3f} ms (min {v['ms_min']:.3f}, max {v['ms_max']:.3f})")
    lines.append(f"- down-converter per station (16 stations, D = 4, u8) over the mono call: {res['ratio']:.2f} "
                 f"(expected about {EXPECTED}, gate {GATE}): " + ("within the gate." if res["ratio"] <= GATE else "ABOVE the gate."))
    lines.append("- Not measured: hardware counters (none were taken), modes 1-3, 51 taps, D other than 4 and 8, "
                 "stereo contexts, host-buffer calls, the CLI.")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide", "bench_wide.json"))
    args = ap.parse_args()
    import torch

    import iqgen

    fm = iqgen.load_fmrx()
    res = {"tool": "tools/bench_wide.py", "mode": 0, "rf_taps": 101, "pairs": PAIRS, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "gate": GATE, "expected": EXPECTED, "hardware_counters": "none taken"}
    with fm.Receiver(0, fm.MONO) as rx:
        u8 = torch.empty(2 * PAIRS, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rx.synth_device(3, 0, PAIRS, u8.data_ptr())
        rx.synchronize()
    s16, f32 = mapped(torch, u8, 2).contiguous(), mapped(torch, u8, 3).contiguous()
    legs = {"mono_call": MonoLeg(fm, torch, u8)}
    for d in (4, 8):
        for n in (1, 16):
            legs[f"ddc_u8_D{d}_x{n}"] = WideLeg(fm, torch, u8, 0, d, n, "ddc")
    for n in (1, 16):
        legs[f"ddc_s16_D4_x{n}"] = WideLeg(fm, torch, s16, 2, 4, n, "ddc")
        legs[f"ddc_f32_D4_x{n}"] = WideLeg(fm, torch, f32, 3, 4, n, "ddc")
    legs["wide_call_u8_D4_x16"] = WideLeg(fm, torch, u8, 0, 4, 16, "call")
    torch.cuda.synchronize()
    res["legs"] = alternate(legs, args.reps)
    res["ratio"] = res["legs"]["ddc_u8_D4_x16"]["ms_median"] / 16 / res["legs"]["mono_call"]["ms_median"]
    res["within_gate"] = res["ratio"] <= GATE
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
