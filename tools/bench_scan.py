#!/usr/bin/env python3
"""Device time of the band scan's spectrum (csrc/scan.hip) against the fused mono receive, on one
device-resident buffer of synthetic mode-0 I/Q:

  scan_1gib   fmrx_scan_spectrum_device, fft_bins 4096, the whole 1 GiB capture
  scan_16mib  the same call on the first 16 MiB (the latency of "what is in this capture?")
  mono_1gib   fmrx_process_device, mode 0, mono, 101-tap RF, on the same 1 GiB (whole blocks)

Each call is timed with a pair of HIP events on the context's stream, after warm-up calls; the
figure is the median of the repeats, the legs alternating in one loop so that drift hits all alike.
The gate: scan_1gib <= 2 x mono_1gib (DESIGN.md §5.6 says why 2 and not 1).  Writes
profiles/scan/bench_scan.json (--out) and exits 1 when the gate is missed.  No counters are read
here: an LDS-bound claim needs a `rocprofv3 --pmc` pass of its own."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

BINS, TAPS, GATE = 4096, 101, 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30, help="capture size (default 1 GiB)")
    ap.add_argument("--small-bytes", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scan", "bench_scan.json"))
    args = ap.parse_args()
    import torch

    import iqgen

    if not torch.cuda.is_available():
        sys.exit("bench_scan.py needs a GPU")
    fm = iqgen.load_fmrx()
    rx = fm.Receiver(0, fm.MONO, rf_taps=TAPS)
    bb = rx.geo.block_bytes
    n_blocks = args.bytes // bb
    iq = torch.empty(args.bytes, dtype=torch.uint8, device="cuda")
    pcm = torch.empty(n_blocks * rx.geo.pcm_samples, dtype=torch.int16, device="cuda")
    power = torch.empty(BINS, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rx.synth_device(3, 0, args.bytes // 2, iq.data_ptr())
    rx.synchronize()
    stream = torch.cuda.ExternalStream(rx.stream())

    def scan_big():
        rx.scan_spectrum_device(iq.data_ptr(), args.bytes // 2, BINS, power.data_ptr())

    def scan_small():
        rx.scan_spectrum_device(iq.data_ptr(), args.small_bytes // 2, BINS, power.data_ptr())

    def mono():
        rx.reset()
        rx.process_device(iq.data_ptr(), n_blocks, pcm.data_ptr())

    legs = {"scan_1gib": scan_big, "scan_16mib": scan_small, "mono_1gib": mono}
    ms = {k: [] for k in legs}
    for r in range(args.warmup + args.reps):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if name == "mono_1gib":
                rx.reset()  # outside the timed window
                rx.synchronize()
                a.record(stream)
                rx.process_device(iq.data_ptr(), n_blocks, pcm.data_ptr())
            else:
                a.record(stream)
                fn()
            b.record(stream)
            rx.synchronize()
            if r >= args.warmup:
                ms[name].append(a.elapsed_time(b))
    spectrum = power.cpu().numpy()
    rx.close()

    def summary(v, nbytes):
        med = statistics.median(v)
        return {"ms_median": med, "ms_min": min(v), "ms_max": max(v), "bytes": nbytes,
                "ms_per_gib": med * (1 << 30) / nbytes, "GB_per_s": nbytes / med / 1e6}

    res = {"tool": "tools/bench_scan.py", "device": torch.cuda.get_device_name(0), "fft_bins": BINS, "rf_taps": TAPS,
           "reps": args.reps, "warmup": args.warmup, "timing": "HIP event pairs on the context stream, median of reps",
           "scan_1gib": summary(ms["scan_1gib"], args.bytes // (2 * BINS) * 2 * BINS),
           "scan_16mib": summary(ms["scan_16mib"], args.small_bytes // (2 * BINS) * 2 * BINS),
           "mono_1gib": summary(ms["mono_1gib"], n_blocks * bb)}
    res["ratio_scan_over_mono"] = res["scan_1gib"]["ms_per_gib"] / res["mono_1gib"]["ms_per_gib"]
    res["gate"] = GATE
    res["within_gate"] = res["ratio_scan_over_mono"] <= GATE
    res["spectrum_sum"] = float(spectrum.astype("float64").sum())  # ~ mean |x|^2: the timed call computed something
    res["not_measured"] = ["hardware counters (LDS busy / bank conflicts, VALU busy): no rocprofv3 --pmc pass",
                           "fft_bins other than 4096", "captures that are not 4-byte aligned"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sys.exit(0 if res["within_gate"] else 1)


if __name__ == "__main__":
    main()
