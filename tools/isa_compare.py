#!/usr/bin/env python3
"""Compare the device code of two gfx950 assembly files symbol by symbol (host only, no GPU).

    hipcc <the Makefile's flags> --offload-device-only -S csrc/X.hip -o X.s
    tools/isa_compare.py PARENT.s THIS.s [--loop REGEX]...

For every kernel and every non-inlined device function of PARENT.s: the instruction text from the
symbol's label to its .Lfunc_end and, for kernels, the .amdhsa_* descriptor block, against the
same symbol in THIS.s.  Only the function number in local labels (.LBB<n>_, .Ltmp<n>, ...) and
`;` comment lines are normalised.  THIS.s may be several translation units concatenated (a file
split): a symbol emitted more than once must match the parent's in every copy.  One markdown table
row a symbol: identical or not, then code bytes, VGPRs, LDS and scratch of PARENT / THIS.
--loop REGEX (may be repeated) adds the instruction count of the smallest loop (a label .. a backward
branch to it) that holds an instruction matching REGEX, for each symbol the first REGEX found in it:
with an instruction only the chain wave issues, the chain's loop body in the PLL runners.
Exit status 1 when a symbol differs or is missing.
"""
import re
import subprocess
import sys

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
LOCAL = re.compile(r"\.L(BB|tmp|func_end|func_begin|JTI|CPI)\d+")
BRANCH = re.compile(r"^\s*s_c?branch\w*\s+(\.LBB_\d+)")


def norm(line):
    line = LOCAL.sub(lambda m: ".L" + m.group(1), line.split(";")[0].rstrip())
    return line


def symbols(path):
    """name -> list of (code lines, descriptor lines, stats dict), one entry a copy."""
    out = {}
    name, code, desc, in_desc = None, [], [], False
    lines = open(path).read().splitlines()
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = LABEL.match(ln)
        if name is None:
            if m and not m.group(1).startswith(".L") and "; @" in ln:
                name, code, desc, in_desc = m.group(1), [], [], False
        elif ln.startswith(".Lfunc_end"):
            stats = {}
            for c in lines[i : i + 40]:
                s = re.match(r"; (codeLenInByte|NumVgprs|ScratchSize|LDSByteSize)\s*[:=]\s*(\d+)", c)
                if s:
                    stats[s.group(1)] = int(s.group(2))
            out.setdefault(name, []).append((code, desc, stats))
            name = None
        else:
            if ".amdhsa_kernel" in ln and ".end_" not in ln:
                in_desc = True
            t = norm(ln)
            if t.strip():
                (desc if in_desc else code).append(t)
            if ".end_amdhsa_kernel" in ln:
                in_desc = False
        i += 1
    return out


def loop_count(code, markers):
    """Instructions of the smallest loop (a label .. a backward branch to it) that holds a line
    matching the first of `markers` found in the symbol at all; None when there is none."""
    pos = {}
    for k, ln in enumerate(code):
        m = re.match(r"^(\.LBB_\d+):", ln)
        if m:
            pos[m.group(1)] = k
    back = []
    for k, ln in enumerate(code):
        m = BRANCH.match(ln)
        if m and m.group(1) in pos and pos[m.group(1)] < k:
            back.append((pos[m.group(1)], k))
    for marker in markers:
        hits = [k for k, ln in enumerate(code) if re.search(marker, ln)]
        if not hits:
            continue
        spans = [(b - a, a, b) for a, b in back if any(a <= k <= b for k in hits)]
        if not spans:
            return None
        _, a, b = min(spans)
        return sum(1 for ln in code[a : b + 1] if ln.startswith("\t") and not ln.lstrip().startswith("."))
    return None


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    args = sys.argv[1:]
    loop = []
    while "--loop" in args:
        k = args.index("--loop")
        loop.append(args[k + 1])
        del args[k : k + 2]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = symbols(args[0]), symbols(args[1])
    nice = demangle(sorted(a))
    bad = 0
    print("| symbol | code and descriptor | code bytes | VGPRs | LDS | scratch |" + (" loop |" if loop else ""))
    print("|---|---|---|---|---|---|" + ("---|" if loop else ""))
    for name in sorted(a, key=lambda n: nice[n]):
        pc, pd, ps = a[name][0]
        short = re.sub(r"fmrx::\(anonymous namespace\)::|\(.*", "", nice[name]).replace("void ", "")
        if name not in b:
            print(f"| `{short}` | MISSING | | | | |")
            bad += 1
            continue
        same = all(c == pc and d == pd for c, d, _ in b[name])
        bad += 0 if same else 1
        desc_same = all(d == pd for _, d, _ in b[name])
        verdict = "identical" if same else ("differs, descriptor unchanged" if desc_same else "DIFFERS, descriptor too")
        if len(b[name]) > 1:
            verdict += f" ({len(b[name])} copies)"
        ts = b[name][0][2]
        col = lambda k: f"{ps.get(k, '-')} / {ts.get(k, '-')}"
        row = f"| `{short}` | {verdict} | {col('codeLenInByte')} | {col('NumVgprs')} | {col('LDSByteSize')} | {col('ScratchSize')} |"
        if loop:
            la, lb = loop_count(pc, loop), loop_count(b[name][0][0], loop)
            row += f" {la} / {lb} |" if la is not None else " |"
        print(row)
    extra = sorted(set(b) - set(a))
    for name in extra:
        print(f"| `{name}` | only in the second file | | | | |")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
