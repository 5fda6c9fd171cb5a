"""CPU side of the external forces (docs/SPEC.md §8): the four entry points are declared, exported and wrapped, and the
driver takes the four new options before it touches the device. No GPU needed."""
import ctypes as C
import os
import subprocess

from abi_header import ROOT, declared_functions

FORCE_SYMBOLS = ("sf_set_vorticity_confinement", "sf_set_buoyancy", "sf_vorticity_magnitude", "sf_add_forces")


def test_force_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in FORCE_SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    for method in ("set_vorticity_confinement", "set_buoyancy", "vorticity_magnitude", "add_forces"):
        assert callable(getattr(solver.FluidSolver, method))


def test_force_entry_points_reject_a_null_context():
    from fluidsolvergpu_amd import solver

    L = solver.lib
    assert L.sf_set_vorticity_confinement(None, C.c_double(0.3)) == solver.SF_ERR_INVALID
    assert L.sf_set_buoyancy(None, C.c_double(1.0), C.c_double(0.0), 1) == solver.SF_ERR_INVALID
    assert L.sf_vorticity_magnitude(None, 0, 1, 2, 8) == solver.SF_ERR_INVALID
    assert L.sf_add_forces(None, 0, 1, 2, 6, 3, 4, 5) == solver.SF_ERR_INVALID


def test_driver_parses_the_force_options_before_the_device():
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    out = subprocess.run([exe, "--vorticity", "0.3", "--buoyancy", "2", "--ambient", "0", "--buoyancy-axis", "1",
                          "--bogus"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (out.returncode, out.stderr)
