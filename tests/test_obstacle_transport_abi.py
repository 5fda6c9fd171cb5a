"""CPU side of sf_set_obstacle_transport / sf_obstacle_transport_get / sf_diffuse_masked / sf_advect_masked
(docs/SPEC.md §17): declared, exported, wrapped, null contexts rejected, and the driver's --obstacle-transport with its
two refusals before the device is touched. No GPU needed."""
import ctypes as C
import os
import subprocess

from abi_header import ROOT, declared_functions

SYMBOLS = ("sf_set_obstacle_transport", "sf_obstacle_transport_get", "sf_diffuse_masked", "sf_advect_masked")
EXE = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
BOX = ("--obstacle", "box:3,3,3:5,5,5", "--pressure", "cg")


def driver(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    for method in ("set_obstacle_transport", "obstacle_transport", "diffuse_masked", "advect_masked"):
        assert callable(getattr(solver.FluidSolver, method))
    assert solver.lib.sf_set_obstacle_transport.argtypes == [C.c_void_p, C.c_int]
    assert solver.lib.sf_obstacle_transport_get.argtypes == [C.c_void_p, C.POINTER(C.c_int)]
    assert solver.lib.sf_diffuse_masked.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double]
    assert solver.lib.sf_advect_masked.argtypes == [C.c_void_p] + [C.c_int] * 6


def test_entry_points_reject_a_null_context_and_a_null_result():
    from fluidsolvergpu_amd import solver

    on = C.c_int(7)
    for value in (0, 1, 2):
        assert solver.lib.sf_set_obstacle_transport(None, value) == solver.SF_ERR_INVALID
    assert solver.lib.sf_obstacle_transport_get(None, C.byref(on)) == solver.SF_ERR_INVALID
    assert on.value == 7
    assert solver.lib.sf_diffuse_masked(None, 0, 6, 7, 1e-4) == solver.SF_ERR_INVALID
    assert solver.lib.sf_advect_masked(None, 0, 6, 7, 0, 1, 2) == solver.SF_ERR_INVALID


def test_driver_takes_obstacle_transport():
    """With --obstacle and --pressure cg the option check passes (the run then needs a device: exit 0 with one, 1
    without); without --obstacle, or with a MacCormack scheme, it is refused with a message."""
    base = ("--n", "8", "--steps", "1", "--every", "0", "--quiet")
    out = driver(*base, *BOX, "--obstacle-transport")
    assert out.returncode in (0, 1) and "unknown option" not in out.stderr and "needs" not in out.stderr, \
        (out.returncode, out.stderr)
    if out.returncode == 1:
        assert "SF_ERR_NO_DEVICE" in out.stderr, out.stderr
    out = driver(*base, "--obstacle-transport")
    assert out.returncode == 2 and "--obstacle-transport needs --obstacle" in out.stderr
    for which in ("vel", "dens", "both"):
        out = driver(*base, *BOX, "--obstacle-transport", "--maccormack", which)
        assert out.returncode == 2 and "does not go with --maccormack" in out.stderr, (which, out.stderr)
    out = driver(*base, *BOX, "--obstacle-transport", "--bogus")
    assert out.returncode == 2 and "unknown option --bogus" in out.stderr
    assert "--obstacle-transport" in driver("--help").stdout + driver("--help").stderr
