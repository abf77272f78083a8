#!/usr/bin/env python3
"""Make tests/golden/stereo_bp.npz: what the reference's own primitives (oracle/_ref/libfmref.so, through
oracle.Reference) give at band-pass lengths other than project.cpp's 51, for machines without the reference.

    python tests/golden/make_stereo_bp.py

  ch_fs<bp_fs>_bp<t>, ca_fs<bp_fs>_bp<t>   impulseResponseBPF's channel (22-54 kHz) and carrier (18.5-19.5 kHz)
                                            tables of t taps at the three band-pass rates of the modes
  demod_m0, demod_m1                        one demod row of 6 blocks in modes 0 and 1 (iqgen.make_rds_demod)
  pcm_sha256_m<mode>_bp<t>                  SHA-256 of the PCM that audio_thread, composed from the reference's
                                            primitives (stereo_ref.audio_compose), makes of that row at t taps

tests/test_stereo_variants_host.py holds the library's design and the oracle's composition to these;
tests/test_gpu_stereo_variants.py runs the rows through the GPU at every length against the hashes."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))

import iqgen  # noqa: E402
import oracle  # noqa: E402
from stereo_ref import BPF_TAPS, audio_compose  # noqa: E402

BP_RATES = (240000, 288000, 256000)
BLOCKS = 6


def main():
    oracle.build()
    ref = oracle.Reference()
    assert ref.own_elementwise, "oracle/_ref/libfmref.so is from an earlier ref_driver.cpp: remove it and build again"
    out = {}
    for fs in BP_RATES:
        for t in BPF_TAPS:
            out[f"ch_fs{fs}_bp{t}"] = ref.bpf(float(fs), 22000.0, 54000.0, t)
            out[f"ca_fs{fs}_bp{t}"] = ref.bpf(float(fs), 18500.0, 19500.0, t)
    for mode in (0, 1):
        demod = iqgen.make_rds_demod(31 + mode, BLOCKS * oracle.MODES[mode][1], oracle.MODES[mode][5])
        out[f"demod_m{mode}"] = demod
        for t in BPF_TAPS:
            pcm = audio_compose(ref, mode, demod, t)["pcm"]
            out[f"pcm_sha256_m{mode}_bp{t}"] = np.array(hashlib.sha256(pcm.tobytes()).hexdigest())
    path = os.path.join(HERE, "stereo_bp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
