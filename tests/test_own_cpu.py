"""sfi::Owned, the owner of a context's device memory, pinned memory, streams and events (csrc/sf_hip.hpp), on the CPU:
tests/own_check.cpp is compiled as a plain C++ program against its own stubs of the HIP runtime (no GPU, no
libamdhip64, no libsfgpu.so) and run. Its failure paths (a throwing constructor, a failing allocation, a repeated lazy
allocation) are exercised here only; no GPU test provokes a failing allocation."""
import os
import subprocess

from abi_header import ROOT


def test_own_check(tmp_path):
    exe = str(tmp_path / "own_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "own_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
