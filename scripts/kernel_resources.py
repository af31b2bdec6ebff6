#!/usr/bin/env python3
"""Kernel resource listing of the HIP translation units, from the compiler's own remarks.

Compiles each .hip file of libfst_amd/csrc for gfx950 with
-Rpass-analysis=kernel-resource-usage (objects are thrown away) and prints one line per
kernel: SGPRs, VGPRs, AGPRs, scratch bytes per lane, spills, waves per SIMD, LDS bytes.

  scripts/kernel_resources.py [--csrc DIR] [files.hip ...] > listing.txt
  scripts/kernel_resources.py --diff old.txt new.txt     # kernels whose figures differ

Template arguments are printed as the demangler gives them, except that the lhs-kind
argument of eager_bfs_kernel / lazy_wave_kernel is normalised (false -> 0, true -> 1), so
listings from before and after that argument became an int compare line by line; likewise
eager_bfs_kernel's fourth argument (lattice emission) and eager_pull_kernel's seventh (weight
codes) are dropped where they are false.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"),
        ("ScratchSize [bytes/lane]", "scratch"), ("SGPRs Spill", "sgpr_spill"),
        ("VGPRs Spill", "vgpr_spill"), ("Occupancy [waves/SIMD]", "waves"),
        ("LDS Size [bytes/block]", "lds")]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return out[:len(names)]


def normalise(name):
    word = {"false": "0", "true": "1"}
    name = re.sub(r"eager_bfs_kernel<(\d+), (false|true)",
                  lambda m: f"eager_bfs_kernel<{m.group(1)}, {word[m.group(2)]}", name)
    # (the emission flag came later still: an instance that does not emit keeps its old name)
    name = re.sub(r"(eager_bfs_kernel<\d+, \d+, \d+), false>", r"\1>", name)
    name = re.sub(r"lazy_wave_kernel<(false|true)>",
                  lambda m: f"lazy_wave_kernel<{word[m.group(1)]}>", name)
    # (eager_pull_kernel's seventh argument, the weight codes: likewise dropped where false)
    name = re.sub(r"(eager_pull_kernel<(?:[^,<>]+, ){5}[^,<>]+), false>", r"\1>", name)
    return re.sub(r"\(.*", "", name)  # the parameter list says nothing the name does not


def listing(csrc, files):
    lines = []
    for f in files:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC",
                   "-ffp-contract=off", "--offload-arch=gfx950",
                   "-Rpass-analysis=kernel-resource-usage", "-c", f, "-o",
                   os.path.join(tmp, "o.o")]
            err = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, check=True).stderr
        kernels, cur = [], None
        for line in err.split("\n"):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = {"name": m.group(1)}
                kernels.append(cur)
                continue
            m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
            if m and cur is not None:
                cur[m.group(1)] = m.group(2)
        names = demangle([k["name"] for k in kernels])
        for k, n in zip(kernels, names):
            figs = " ".join(f"{short}={k.get(key, '?')}" for key, short in KEYS)
            lines.append(f"{f}: {normalise(n)} | {figs}")
    return sorted(lines)


def diff(a, b):
    def load(p):
        d = {}
        for line in open(p):
            if " | " in line:
                k, v = line.rstrip("\n").split(" | ")
                d[k] = v
        return d
    da, db = load(a), load(b)
    bad = 0
    for k in sorted(da):
        if k not in db:
            print(f"gone: {k}")
            bad += 1
        elif da[k] != db[k]:
            print(f"changed: {k}\n  {da[k]}\n  {db[k]}")
            bad += 1
    for k in sorted(db):
        if k not in da:
            print(f"new: {k} | {db[k]}")
    print(f"{len(da)} kernels compared, {bad} changed or gone")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(REPO, "libfst_amd", "csrc"))
    ap.add_argument("--diff", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    if a.diff:
        sys.exit(diff(*a.diff))
    files = a.files or sorted(f for f in os.listdir(a.csrc) if f.endswith(".hip"))
    print("\n".join(listing(a.csrc, files)))


if __name__ == "__main__":
    main()
