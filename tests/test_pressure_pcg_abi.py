"""CPU side of sf_set_pressure_preconditioner / sf_pressure_preconditioner_get (docs/SPEC.md §11.2): declared, exported,
wrapped, the struct and the enum as the header has them, sf_pressure_info's layout untouched, and the driver's option
parsed before the device is touched. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

from abi_header import ROOT, declared_functions, header_text, struct_members

SYMBOLS = ("sf_set_pressure_preconditioner", "sf_pressure_preconditioner_get")


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    assert callable(solver.FluidSolver.set_pressure_preconditioner)
    assert isinstance(solver.FluidSolver.pressure_preconditioner, property)
    assert solver.lib.sf_set_pressure_preconditioner.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert solver.lib.sf_pressure_preconditioner_get.argtypes == [C.c_void_p, C.POINTER(solver.SfPressurePreconditioner)]


def test_struct_and_enum_match_the_header():
    from fluidsolvergpu_amd import solver

    members = struct_members(header_text(), "sf_pressure_preconditioner")
    assert members == [("kind", "int"), ("sweeps", "int")]
    assert [(n, C.c_int) for n, _ in members] == list(solver.SfPressurePreconditioner._fields_)
    assert C.sizeof(solver.SfPressurePreconditioner) == 8
    enum = re.search(r"enum\s+sf_pressure_precond\s*\{([^}]*)\}", header_text()).group(1)
    assert [e.strip() for e in enum.split(",")] == ["SF_PRECOND_NONE = 0", "SF_PRECOND_JACOBI = 1"]
    assert (solver.SF_PRECOND_NONE, solver.SF_PRECOND_JACOBI) == (0, 1)
    assert solver.PRECONDITIONERS == {"none": 0, "jacobi": 1}
    # sf_pressure_info stays exactly as it is
    assert struct_members(header_text(), "sf_pressure_info") == [
        ("solver", "int"), ("status", "int"), ("iterations", "int"), ("rel_residual", "double"),
        ("solves_total", "long long"), ("iterations_total", "long long")]
    assert C.sizeof(solver.SfPressureInfo) == 40


def test_entry_points_reject_a_null_context_and_a_null_result():
    from fluidsolvergpu_amd import solver

    out = solver.SfPressurePreconditioner()
    assert solver.lib.sf_set_pressure_preconditioner(None, solver.SF_PRECOND_JACOBI, 4) == solver.SF_ERR_INVALID
    assert solver.lib.sf_set_pressure_preconditioner(None, solver.SF_PRECOND_NONE, 0) == solver.SF_ERR_INVALID
    assert solver.lib.sf_pressure_preconditioner_get(None, C.byref(out)) == solver.SF_ERR_INVALID


def test_driver_parses_pressure_precond_before_the_device():
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    for spec in ("none", "jacobi:1", "jacobi:4", "jacobi:12"):
        out = subprocess.run([exe, "--pressure", "cg:1e-3:40", "--pressure-precond", spec, "--bogus"],
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (spec, out.returncode, out.stderr)
    for spec in ("", "jacobi", "jacobi:", "jacobi:0", "jacobi:-2", "jacobi:2.5", "jacobi:3x", "jacobi:+3", "jacobi:4:1",
                 "none:4", "cheb:4", "4"):
        out = subprocess.run([exe, "--pressure-precond", spec], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--pressure-precond takes" in out.stderr, (spec, out.returncode, out.stderr)
    # --pressure keeps its grammar
    out = subprocess.run([exe, "--pressure", "cg:1e-3:40:jacobi", "--bogus"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "unknown option --bogus" not in out.stderr, (out.returncode, out.stderr)
