"""CPU side of sf_set_pressure_multigrid / sf_pressure_multigrid_get / sf_precondition (docs/SPEC.md §11.3): declared,
exported, wrapped, the struct as the header has it, the preconditioner enum of §11.2 untouched, and the driver's option
parsed before the device is touched. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

from abi_header import ROOT, declared_functions, header_text, struct_members

SYMBOLS = ("sf_set_pressure_multigrid", "sf_pressure_multigrid_get", "sf_precondition")


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    assert callable(solver.FluidSolver.set_pressure_multigrid)
    assert callable(solver.FluidSolver.precondition)
    assert isinstance(solver.FluidSolver.pressure_multigrid, property)
    assert solver.lib.sf_set_pressure_multigrid.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int]
    assert solver.lib.sf_pressure_multigrid_get.argtypes == [C.c_void_p, C.POINTER(solver.SfPressureMultigrid)]
    assert solver.lib.sf_precondition.argtypes == [C.c_void_p, C.c_int, C.c_int]
    import inspect

    sig = inspect.signature(solver.FluidSolver.set_pressure_multigrid)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("sweeps", inspect.Parameter.empty), ("max_levels", 0), ("coarse_sweeps", 8)]


def test_struct_matches_the_header():
    from fluidsolvergpu_amd import solver

    members = struct_members(header_text(), "sf_pressure_multigrid")
    assert members == [("sweeps", "int"), ("max_levels", "int"), ("coarse_sweeps", "int"), ("levels", "int")]
    assert [(n, C.c_int) for n, _ in members] == list(solver.SfPressureMultigrid._fields_)
    assert C.sizeof(solver.SfPressureMultigrid) == 16


def test_the_preconditioner_enum_and_names_read_as_before():
    from fluidsolvergpu_amd import solver

    enum = re.search(r"enum\s+sf_pressure_precond\s*\{([^}]*)\}", header_text()).group(1)
    assert [e.strip() for e in enum.split(",")] == ["SF_PRECOND_NONE = 0", "SF_PRECOND_JACOBI = 1"]
    assert solver.PRECONDITIONERS == {"none": 0, "jacobi": 1}
    assert struct_members(header_text(), "sf_pressure_preconditioner") == [("kind", "int"), ("sweeps", "int")]
    assert C.sizeof(solver.SfPressureInfo) == 40


def test_entry_points_reject_a_null_context_and_a_null_result():
    from fluidsolvergpu_amd import solver

    out = solver.SfPressureMultigrid()
    assert solver.lib.sf_set_pressure_multigrid(None, 2, 0, 8) == solver.SF_ERR_INVALID
    assert solver.lib.sf_set_pressure_multigrid(None, 0, 0, 8) == solver.SF_ERR_INVALID
    assert solver.lib.sf_pressure_multigrid_get(None, C.byref(out)) == solver.SF_ERR_INVALID
    assert solver.lib.sf_precondition(None, 0, 1) == solver.SF_ERR_INVALID


def test_driver_parses_pressure_mg_before_the_device():
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    for spec in ("2", "2:0:8", "1:3"):
        out = subprocess.run([exe, "--pressure", "cg:1e-3:40", "--pressure-mg", spec, "--bogus"],
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (spec, out.returncode, out.stderr)
    for spec in ("", "0", "mg", "2:", "2:-1", "2:0:0", "2:0:8:1", "2.5"):
        out = subprocess.run([exe, "--pressure-mg", spec], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and out.stderr.startswith("--pressure-mg takes"), (spec, out.returncode, out.stderr)
    # --pressure-precond keeps its grammar next to it
    out = subprocess.run([exe, "--pressure-precond", "jacobi:4", "--pressure-mg", "2", "--bogus"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (out.returncode, out.stderr)
