"""CPU side of sf_set_pressure_sync / sf_pressure_sync_get (docs/SPEC.md §11 "Where the scalars are computed"): declared,
exported, wrapped, the struct as the header has it, sf_pressure_info's layout untouched, and the driver's option parsed
before the device is touched. No GPU needed."""
import ctypes as C
import os
import subprocess

from abi_header import ROOT, declared_functions, header_text, struct_members

SYMBOLS = ("sf_set_pressure_sync", "sf_pressure_sync_get")
CTYPES = {"int": C.c_int, "long long": C.c_longlong, "double": C.c_double}


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    assert callable(solver.FluidSolver.set_pressure_sync)
    assert isinstance(solver.FluidSolver.pressure_sync, property)
    assert solver.lib.sf_set_pressure_sync.argtypes == [C.c_void_p, C.c_int]
    assert solver.lib.sf_pressure_sync_get.argtypes == [C.c_void_p, C.POINTER(solver.SfPressureSync)]


def test_structs_match_the_header():
    from fluidsolvergpu_amd import solver

    members = struct_members(header_text(), "sf_pressure_sync")
    assert members == [("check_every", "int"), ("host_waits", "int"), ("host_waits_total", "long long")]
    assert [(n, CTYPES[t]) for n, t in members] == list(solver.SfPressureSync._fields_)
    assert C.sizeof(solver.SfPressureSync) == 16
    # sf_pressure_info keeps its layout
    assert struct_members(header_text(), "sf_pressure_info") == [
        ("solver", "int"), ("status", "int"), ("iterations", "int"), ("rel_residual", "double"),
        ("solves_total", "long long"), ("iterations_total", "long long")]
    assert C.sizeof(solver.SfPressureInfo) == 40


def test_entry_points_reject_a_null_context_and_a_null_result():
    from fluidsolvergpu_amd import solver

    out = solver.SfPressureSync()
    assert solver.lib.sf_set_pressure_sync(None, 4) == solver.SF_ERR_INVALID
    assert solver.lib.sf_pressure_sync_get(None, C.byref(out)) == solver.SF_ERR_INVALID


def test_driver_parses_pressure_sync_before_the_device():
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    for m in ("0", "1", "8", "1000"):
        out = subprocess.run([exe, "--pressure", "cg:1e-3:40", "--pressure-sync", m, "--bogus"], capture_output=True,
                             text=True, timeout=60)
        assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (m, out.returncode, out.stderr)
    for m in ("-1", "", "four", "2.5", "3x"):
        out = subprocess.run([exe, "--pressure-sync", m], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--pressure-sync takes" in out.stderr, (m, out.returncode, out.stderr)
