"""CPU side of volume rendering and light marching (docs/SPEC.md §12): the three entry points are declared, exported
and wrapped, sf_render_params agrees between include/sfgpu.h and the ctypes mirror, and the driver takes --render before
it touches the device. No GPU needed."""
import ctypes as C
import os
import subprocess

from abi_header import ROOT, declared_functions, header_text, struct_members

SYMBOLS = ("sf_render", "sf_render_read", "sf_light")
EXE = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    for method in ("render", "light"):
        assert callable(getattr(solver.FluidSolver, method))


def test_struct_layout_matches_the_header():
    from fluidsolvergpu_amd import solver

    members = struct_members(header_text(), "sf_render_params")
    assert members == [("axis", "int"), ("from_high", "int"), ("sigma", "double"), ("dens", "int"), ("emit", "int")]
    want = {"int": C.c_int, "double": C.c_double}
    assert [(n, t) for n, t in solver.SfRenderParams._fields_] == [(n, want[t]) for n, t in members]
    assert C.sizeof(solver.SfRenderParams) == 24
    assert [getattr(solver.SfRenderParams, n).offset for n, _ in members] == [0, 4, 8, 16, 20]


def test_entry_points_reject_a_null_context():
    from fluidsolvergpu_amd import solver

    p = solver.SfRenderParams(axis=0, from_high=0, sigma=1.0, dens=6, emit=-1)
    assert solver.lib.sf_render(None, C.byref(p)) == solver.SF_ERR_INVALID
    assert solver.lib.sf_render_read(None, None, None) == solver.SF_ERR_INVALID
    assert solver.lib.sf_light(None, 8, 6, 0, 0, 1.0) == solver.SF_ERR_INVALID


def test_driver_parses_render_before_the_device():
    for good in ("i+:0", "j-:4", "k+:2.5:i-", "j+:4:k-"):
        out = subprocess.run([EXE, "--render", good, "--bogus"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (good, out.returncode, out.stderr)
    for bad in ("", "j+", "j:4", "x+:4", "j+:", "j+:-1", "j+:nan", "j+:inf", "j+:4x", "j+:4:", "j+:4:k", "j+:4:k-:1",
                "jj+:4", "4:j+"):
        out = subprocess.run([EXE, "--render", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--render takes VIEW:SIGMA[:LIGHT]" in out.stderr, (bad, out.returncode, out.stderr)
    out = subprocess.run([EXE, "--render"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "missing value" in out.stderr, (out.returncode, out.stderr)


def test_driver_lists_render_in_its_usage():
    out = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--render VIEW:SIGMA[:LIGHT]" in out.stdout, (out.returncode, out.stdout)
    out = subprocess.run([EXE, "--bogus"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--render VIEW:SIGMA[:LIGHT]" in out.stderr
