#!/usr/bin/env python3
"""Make tests/golden/drivers_parent.json: what the two drivers, fmrx.decode_stations and the fmrx executable
(csrc/cli.cpp), do at the commit before they were restructured, recorded on an MI355X.

    python tests/golden/make_drivers_parent.py [--out PATH] [--head COMMIT,FMRX_BLOB,CLI_BLOB]

The record is written once, from the parent's two files, and never again: the restructured drivers are
measured against it, not the other way round.  So the script refuses to write unless fmrx.py and
csrc/cli.cpp are byte for byte the blobs of HEAD.  In a git work tree it asks git for HEAD and the two
blob ids; a tree that was copied without its history to the machine with the GPU is given the same three
ids by --head (`git rev-parse HEAD HEAD:<fmrx.py> HEAD:<csrc/cli.cpp>`, joined by commas).

Only public names are used: decode_stations and bin/fmrx (tests/drivers_ref.py holds the cases and the
serialisation, shared with tests/test_gpu_drivers.py and tests/test_drivers_host.py).  Sections:
  captures    SHA-256 of every input's bytes (the tests assert these first: a drifting generator is told
              apart from a drifting decode)
  decode      21 decode_stations cases: the tuple's length, the stations, the PCM, every further element
  cli         6 runs of the executable: exit status, the whole stderr, length and SHA-256 of stdout
  refusals    10 argument lists the executable refuses before it opens a context: exit status and stderr
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import drivers_ref as D  # noqa: E402
import iqgen  # noqa: E402

DRIVERS = ("software-defined-radio-course-project_amd/fmrx.py", "software-defined-radio-course-project_amd/csrc/cli.cpp")


def blob_id(path: str) -> str:
    """The id git gives the file's bytes as a blob."""
    data = open(os.path.join(REPO, path), "rb").read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def head_ids(given):
    if given:
        ids = given.split(",")
    else:
        ids = subprocess.run(["git", "rev-parse", "HEAD"] + [f"HEAD:{p}" for p in DRIVERS], cwd=REPO, check=True,
                             capture_output=True, text=True).stdout.split()
    if len(ids) != 3 or any(len(i) != 40 for i in ids):
        sys.exit("need HEAD's commit id and the blob ids of fmrx.py and csrc/cli.cpp")
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=D.RECORD)
    ap.add_argument("--head")
    args = ap.parse_args()
    commit, *blobs = head_ids(args.head)
    for path, want in zip(DRIVERS, blobs):
        if blob_id(path) != want:
            sys.exit(f"{path} differs from HEAD ({commit}): the record is made from the parent's drivers alone")
    fm = iqgen.load_fmrx()
    rec = {"commit": commit, "drivers": dict(zip(DRIVERS, blobs)), "captures": D.capture_hashes(), "decode": {}, "cli": {},
           "refusals": {}}
    for section, names, run in (("decode", D.DECODE_CASES, D.decode_case), ("cli", D.CLI_CASES, D.cli_case)):
        for name in names:
            t0 = time.perf_counter()
            rec[section][name] = run(fm, name)
            print(f"{section} {name}: {time.perf_counter() - t0:.2f} s  {D.text(rec[section][name])[:200]}", flush=True)
    for argv in D.REFUSALS:
        rec["refusals"][" ".join(argv)] = D.refusal_case(fm, argv)
        print("refusal", argv, rec["refusals"][" ".join(argv)], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
