"""tests/drivers_ref.py — helper of the drivers' tests (not a test).

The cases of tests/golden/drivers_parent.json, how each is run and how its result is written down.  The
record was made by tests/golden/make_drivers_parent.py at the commit before fmrx.decode_stations and
csrc/cli.cpp were restructured; tests/test_gpu_drivers.py and tests/test_drivers_host.py run the same cases
through the same functions and compare the canonical JSON text, so nothing here depends on how either
driver is written, only on decode_stations' arguments and result and on the fmrx executable's arguments,
streams and exit status.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess

import numpy as np

import afc_ref as A

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drivers_parent.json")
SHORT = 23 * 12800  # capture B: less than one frame (24 blocks) of capture A

# ---- a. decode_stations: case -> (capture, channels, keyword arguments) ----------------------------------
DECODE_CASES = {
    "A1": ("A", "MONO", {}),
    "A2": ("A", "MONO", dict(rds=True)),
    "A3": ("A", "MONO", dict(rds=True, rds_sync=True)),
    "A4": ("A", "STEREO", {}),
    "A5": ("A", "STEREO", dict(blend=True)),
    "A6": ("A", "MONO", dict(probe=True)),
    "A7": ("A", "STEREO", dict(rds=True, probe=True)),
    "A8": ("A", "STEREO", dict(probe=True, blend=True)),
    "A9": ("A", "MONO", dict(afc=True)),
    "A10": ("A", "MONO", dict(probe=True, afc=True)),
    "A11": ("A", "STEREO", dict(rds=True, blend=True, afc=True)),
    "A12": ("A", "STEREO", dict(rds=True, rds_sync=True, probe=True, blend=True, afc=True, deemphasis_us=50)),
    "A13": ("A", "MONO", dict(deemphasis_us=75)),
    "B1": ("B", "MONO", dict(probe=True, fft_bins=4096)),
    "B2": ("B", "MONO", dict(afc=True, fft_bins=4096)),
    "B3": ("B", "STEREO", dict(probe=True, blend=True, afc=True, fft_bins=4096)),
    "C1": ("C", "MONO", {}),
    "C2": ("C", "MONO", dict(rds=True)),
    "C3": ("C", "STEREO", dict(rds=True, probe=True, blend=True, afc=True)),
    "D1": ("decim2", "MONO", dict(capture_decim=2, rds=True, probe=True, afc=True)),
    "D2": ("rate", "STEREO", dict(capture_rate=10000000, blend=True, afc=True)),
}

# ---- b. the executable on the GPU: case -> (input, arguments) ----------------------------------------------
CLI_CASES = {
    "R1": ("A+tail", ["0", "2", "--offset-hz", "100000"]),
    "R2": ("A+tail", ["0", "2", "--offset-hz", "-600000", "--rds", "--rds-sync", "--meter", "--blend", "--afc", "--deemph", "50"]),
    "R3": ("A+tail", ["0", "1", "--mono-product", "--meter", "--afc"]),
    "R4": ("A+tail", ["0", "2", "--rds", "--batch", "100"]),  # 100 blocks round up to 5 granules of 24
    "R5": ("decim2+tail", ["0", "2", "--capture-decim", "2", "--offset-hz", str(A.TUNED[0]), "--meter", "--afc"]),
    "R6": ("A+tail", ["--scan"]),
}

# ---- c. refusals that leave before a context exists (no GPU) -------------------------------------------------
REFUSALS = [
    ["0", "2", "--rds-sync"],
    ["0", "1", "--blend"],
    ["0", "2", "--blend", "--mono-product"],
    ["--iq-format", "x"],
    ["--capture-decim", "11"],
    ["--capture-decim", "0"],
    ["--capture-rate", "4800000", "--capture-decim", "2"],
    ["--capture-rate", "0"],
    ["--deemph", "60"],
    ["--offset-hz"],
]

CAPTURES = ("A", "B", "C", "decim2", "rate", "A+tail", "decim2+tail")
_cache = {}


def capture(name: str) -> np.ndarray:
    """A named input, u8: A is afc_ref.shifted_capture5() (mode 0, three stations, 20 frames), B its first 23
    blocks, C the station-less capture of test_gpu_scan.test_decode_stations, decim2 and rate
    afc_ref.tracking_capture's; +tail: five blocks of 0x80 behind it, as test_gpu_afc.test_cli_afc_line pads."""
    if name not in _cache:
        if name.endswith("+tail"):
            blocks = 5 * 12800 * (2 if name.startswith("decim2") else 1)
            _cache[name] = np.concatenate([capture(name[:-5]), np.full(blocks, 128, np.uint8)])
        elif name == "A":
            _cache[name] = A.shifted_capture5()
        elif name == "B":
            _cache[name] = capture("A")[:SHORT]
        elif name == "C":
            from test_scan_host import capture as scan_capture

            _cache[name] = scan_capture("rand")[0]
        else:
            _cache[name] = A.tracking_capture(name)
    return _cache[name]


def sha256(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def capture_hashes() -> dict:
    return {name: sha256(capture(name)) for name in CAPTURES}


def canon(x):
    """x as JSON that loses nothing: floats through repr, arrays as shape, dtype and SHA-256 of their bytes, a
    station as its three fields, None, bool, int, str, lists and dicts as they are."""
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, float):
        return {"float": repr(x)}
    if isinstance(x, np.generic):
        return {"numpy": str(x.dtype), "value": canon(x.item())}
    if isinstance(x, np.ndarray):
        return {"shape": list(x.shape), "dtype": str(x.dtype), "sha256": sha256(x)}
    if isinstance(x, dict):
        return {"dict": {str(k): canon(v) for k, v in x.items()}}
    if isinstance(x, tuple):
        return {"tuple": [canon(v) for v in x]}
    if isinstance(x, list):
        return [canon(v) for v in x]
    if hasattr(x, "offset_hz") and hasattr(x, "snr_db"):  # fmrx.Station
        return {"offset_hz": int(x.offset_hz), "power_db": repr(float(x.power_db)), "snr_db": repr(float(x.snr_db))}
    raise TypeError(f"no canonical form for {type(x).__name__}")


def text(x) -> str:
    """The canonical JSON text two results are compared by (NaN-safe: every float is a string)."""
    return json.dumps(x, sort_keys=True)


def decode_case(fm, name: str) -> dict:
    """One decode_stations case: the tuple's length, the stations, the PCM array and every further element;
    a raised exception as its type's name."""
    cap, channels, kw = DECODE_CASES[name]
    try:
        res = fm.decode_stations(capture(cap), 0, getattr(fm, channels), **kw)
    except Exception as e:  # what is recorded is that it raises, and what; a HIP error is no behaviour to record
        if getattr(e, "code", None) == fm.FMRX_EHIP:
            raise
        return {"raises": type(e).__name__}
    return {"len": len(res), "stations": canon(res[0]), "pcm": canon(res[1]), "rest": [canon(e) for e in res[2:]]}


def exe_of(fm) -> str:
    return os.path.join(os.path.dirname(fm.LIB_PATH), "bin", "fmrx")


def run_cli(fm, args, data: bytes, timeout: int = 120):
    """The executable as `fmrx <args>` (the usage text prints its own name) with data on stdin."""
    return subprocess.run(["fmrx"] + list(args), executable=exe_of(fm), input=data, capture_output=True, timeout=timeout)


def cli_case(fm, name: str) -> dict:
    cap, args = CLI_CASES[name]
    r = run_cli(fm, args, capture(cap).tobytes())
    if r.returncode < 0:
        raise RuntimeError(f"fmrx {' '.join(args)} died of signal {-r.returncode}: {r.stderr.decode()}")
    return {"status": r.returncode, "stderr": r.stderr.decode(), "stdout_bytes": len(r.stdout),
            "stdout_sha256": hashlib.sha256(r.stdout).hexdigest()}


def refusal_case(fm, args) -> dict:
    r = run_cli(fm, args, b"", timeout=30)
    return {"status": r.returncode, "stderr": r.stderr.decode(), "stdout_bytes": len(r.stdout)}


def load_record() -> dict:
    with open(RECORD) as f:
        return json.load(f)
