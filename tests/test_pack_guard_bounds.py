"""The guard bands of tier P's packed cells, swept on the CPU: builds tools/pack_guard_check.cpp
(host C++ over kernels/pull_window.hpp, the header the kernel and the host gate share) and runs
it.  The program checks every cell offset a window row can form against the padded array; see
its header comment for the sweep."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "libfst_amd", "tools", "pack_guard_check.cpp")


def test_pack_guard_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/bin/hipcc"):
        cxx = "/opt/rocm/bin/hipcc"
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "pack_guard_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-x", "c++", SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "pack_guard_check: ok"
