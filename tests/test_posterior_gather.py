"""The shard gather of fst_posterior_lhs_batch, on the CPU under AddressSanitizer and UBSan:
builds tools/posterior_gather_check.cpp (host C++ over csrc/posterior_gather.hpp, the header the
entry itself uses) with -fsanitize=address,undefined as a program of its own and runs it.  The
program gathers random shard plans into result arrays of exactly the caller's extents; see its
header comment.  Nothing sanitised is loaded into Python."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "libfst_amd", "tools", "posterior_gather_check.cpp")


def test_posterior_gather_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "posterior_gather_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all", "-x", "c++", SRC, "-o", exe]
    # the runtimes linked into the program (gcc's default is shared; clang's is static already),
    # so that it starts the same whatever else the process environment loads first
    if subprocess.run(base + ["-static-libasan", "-static-libubsan"],
                      capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "posterior_gather_check: ok"
