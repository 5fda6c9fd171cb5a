"""CPU side of the conjugate-gradient projection (docs/SPEC.md §11): the four entry points are declared, exported and
wrapped, and the driver takes --pressure before it touches the device. No GPU needed."""
import os
import subprocess

from abi_header import ROOT, declared_functions, enum_values, header_text, struct_field_names

SYMBOLS = ("sf_set_pressure_solver", "sf_project_cg", "sf_poisson_residual", "sf_pressure_info_get")


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    for method in ("set_pressure_solver", "project_cg", "poisson_residual", "pressure_info"):
        assert callable(getattr(solver.FluidSolver, method))
    for enum, want in (("sf_pressure_solver", {"SF_PRESSURE_JACOBI": "0", "SF_PRESSURE_CG": "1"}),
                       ("sf_cg_status", {"SF_CG_CONVERGED": "0", "SF_CG_MAX_ITERS": "1", "SF_CG_BREAKDOWN": "2"})):
        assert enum_values(header_text(), enum) == want
    assert (solver.SF_PRESSURE_JACOBI, solver.SF_PRESSURE_CG) == (0, 1)
    assert (solver.SF_CG_CONVERGED, solver.SF_CG_MAX_ITERS, solver.SF_CG_BREAKDOWN) == (0, 1, 2)


def test_info_struct_matches_the_header():
    import ctypes as C

    from fluidsolvergpu_amd import solver

    assert struct_field_names(header_text(), "sf_pressure_info") == [n for n, _ in solver.SfPressureInfo._fields_]
    kinds = dict(solver.SfPressureInfo._fields_)
    assert kinds["rel_residual"] is C.c_double and kinds["iterations_total"] is C.c_longlong and kinds["solver"] is C.c_int


def test_entry_points_reject_a_null_context():
    import ctypes as C

    from fluidsolvergpu_amd import solver

    L = solver.lib
    out = C.c_double()
    info = solver.SfPressureInfo()
    assert L.sf_set_pressure_solver(None, 1, 1e-3, 10) == solver.SF_ERR_INVALID
    assert L.sf_project_cg(None, 0, 1, 2, 3, 4, 1e-3, 10) == solver.SF_ERR_INVALID
    assert L.sf_poisson_residual(None, 3, 4, C.byref(out)) == solver.SF_ERR_INVALID
    assert L.sf_pressure_info_get(None, C.byref(info)) == solver.SF_ERR_INVALID


def test_driver_parses_pressure_before_the_device():
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    for spec in ("jacobi", "cg", "cg:1e-2", "cg:5e-4:40", "cg:1e-3:0"):
        out = subprocess.run([exe, "--pressure", spec, "--bogus"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (spec, out.returncode, out.stderr)
    for spec in ("bogus", "cg:", "cg:0", "cg:-1e-3", "cg:nan", "cg:inf", "cg:1e-3:", "cg:1e-3:-1", "cg:1e-3:ten", "cg:1e-3:5:6",
                 "jacobi:1e-3", "cgx"):
        out = subprocess.run([exe, "--pressure", spec], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--pressure takes jacobi or cg[:tol[:max_iters]]" in out.stderr, (spec, out.returncode, out.stderr)
    out = subprocess.run([exe, "--pressure"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "missing value" in out.stderr, (out.returncode, out.stderr)
