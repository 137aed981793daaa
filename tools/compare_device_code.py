#!/usr/bin/env python3
"""Is the device code of two builds the same, kernel by kernel?  For a change that should touch host code only.
   hipcc <the library's flags> --cuda-device-only -S -o a.s celeste_hip.hip    (once per tree)
   python tools/compare_device_code.py a.s b.s
Each listing is cut at its kernels (from the symbol to .end_amdhsa_kernel: the instructions and the .amdhsa_ block); the
function ordinal in the local labels (.LBB<f>_<n>, .Lfunc_end<f>) numbers the functions in emission order and is rewritten,
and runs of blanks are folded (a label's comment column moves with the ordinal's digits).  Exit status 1 when a kernel differs."""
import hashlib, re, sys


def kernels(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    start = {}
    for i, l in enumerate(lines):
        m = re.match(r"(\S+):", l)
        if m and m.group(1) in names and m.group(1) not in start:
            start[m.group(1)] = i
    out = {}
    for n in names:
        end = next(j for j in range(start[n], len(lines)) if lines[j].strip().startswith(".end_amdhsa_kernel"))
        t = "\n".join(lines[start[n] + 1:end + 1])
        t = re.sub(r"BB\d+_", "BBf_", re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1f", t))
        out[n] = hashlib.sha256(re.sub(r"[ \t]+", " ", t).encode()).hexdigest()
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
both = [n for n in a if n in b]
differ = [n for n in both if a[n] != b[n]]
print("kernels: %d and %d; compared %d, equal %d" % (len(a), len(b), len(both), len(both) - len(differ)))
print("differ: %s\nonly in the first: %s\nonly in the second: %s" % (differ, [n for n in a if n not in b], [n for n in b if n not in a]))
sys.exit(1 if differ else 0)
