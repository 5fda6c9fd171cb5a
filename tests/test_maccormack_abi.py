"""CPU side of MacCormack advection (docs/SPEC.md §9): the two entry points are declared, exported and wrapped, and the
driver takes --maccormack before it touches the device. No GPU needed."""
import os
import subprocess

from abi_header import ROOT, declared_functions, enum_values, header_text

SYMBOLS = ("sf_set_advection", "sf_advect_maccormack")


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    for method in ("set_advection", "advect_maccormack"):
        assert callable(getattr(solver.FluidSolver, method))
    assert enum_values(header_text(), "sf_advection") == {"SF_ADVECT_SEMI_LAGRANGIAN": "0", "SF_ADVECT_MACCORMACK": "1"}
    assert (solver.SF_ADVECT_SEMI_LAGRANGIAN, solver.SF_ADVECT_MACCORMACK) == (0, 1)


def test_entry_points_reject_a_null_context():
    from fluidsolvergpu_amd import solver

    L = solver.lib
    assert L.sf_set_advection(None, 1, 1) == solver.SF_ERR_INVALID
    assert L.sf_advect_maccormack(None, 0, 6, 7, 0, 1, 2) == solver.SF_ERR_INVALID


def test_driver_parses_maccormack_before_the_device():
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    for which in ("vel", "dens", "both"):
        out = subprocess.run([exe, "--maccormack", which, "--bogus"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (out.returncode, out.stderr)
    out = subprocess.run([exe, "--maccormack", "bogus"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--maccormack takes vel, dens or both" in out.stderr, (out.returncode, out.stderr)
    out = subprocess.run([exe, "--maccormack"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "missing value" in out.stderr, (out.returncode, out.stderr)
