"""CPU side of the reductions and diagnostics (docs/SPEC.md §10): the entry points are declared, exported and wrapped,
the enum and the struct agree between include/sfgpu.h and the ctypes mirror, and the driver takes --monitor before it
touches the device. No GPU needed."""
import ctypes as C
import os
import subprocess

from abi_header import ROOT, declared_functions, enum_values, header_text, struct_members

SYMBOLS = ("sf_reduce", "sf_diagnostics_get")
OPS = {"SF_RED_SUM": 0, "SF_RED_SUM_SQ": 1, "SF_RED_MIN": 2, "SF_RED_MAX": 3, "SF_RED_MAX_ABS": 4,
       "SF_RED_COUNT_NONFINITE": 5}
DOUBLES = ["mass", "dens_min", "dens_max", "kinetic", "max_speed", "max_div", "cfl_x", "cfl_y", "cfl_z", "cfl"]


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    for method in ("reduce", "diagnostics"):
        assert callable(getattr(solver.FluidSolver, method))


def test_enum_values():
    from fluidsolvergpu_amd import solver

    assert {k: int(v) for k, v in enum_values(header_text(), "sf_reduce_op").items()} == OPS
    for name, value in OPS.items():
        assert getattr(solver, name) == value
    assert sorted(solver.REDUCE_OPS.values()) == list(range(6))


def test_struct_layout_matches_the_header():
    from fluidsolvergpu_amd import solver

    members = struct_members(header_text(), "sf_diagnostics")
    assert members == [(n, "double") for n in DOUBLES] + [("nonfinite", "long long")]
    want = {"double": C.c_double, "long long": C.c_longlong}
    assert [(n, t) for n, t in solver.SfDiagnostics._fields_] == [(n, want[t]) for n, t in members]
    assert C.sizeof(solver.SfDiagnostics) == 8 * 11
    for q, (n, _) in enumerate(members):
        assert getattr(solver.SfDiagnostics, n).offset == 8 * q


def test_entry_points_reject_a_null_context():
    from fluidsolvergpu_amd import solver

    out, d = C.c_double(), solver.SfDiagnostics()
    assert solver.lib.sf_reduce(None, 0, 6, C.byref(out)) == solver.SF_ERR_INVALID
    assert solver.lib.sf_diagnostics_get(None, C.byref(d)) == solver.SF_ERR_INVALID


def test_driver_parses_monitor_before_the_device():
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    out = subprocess.run([exe, "--monitor", "5", "--bogus"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (out.returncode, out.stderr)
    for bad in ("0", "-3", "often"):
        out = subprocess.run([exe, "--monitor", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--monitor takes a step count >= 1" in out.stderr, (out.returncode, out.stderr)
    out = subprocess.run([exe, "--monitor"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "missing value" in out.stderr, (out.returncode, out.stderr)
