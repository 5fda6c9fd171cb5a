"""CPU side of sf_set_obstacle_maccormack / sf_obstacle_maccormack_get / sf_advect_maccormack_masked (docs/SPEC.md §18):
declared, exported, wrapped, null contexts and a null result pointer rejected, and the driver's --obstacle-maccormack
with its outcomes before the device is touched. No GPU needed."""
import ctypes as C
import os
import subprocess

from abi_header import ROOT, declared_functions

SYMBOLS = ("sf_set_obstacle_maccormack", "sf_obstacle_maccormack_get", "sf_advect_maccormack_masked")
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
    for method in ("set_obstacle_maccormack", "obstacle_maccormack", "advect_maccormack_masked"):
        assert callable(getattr(solver.FluidSolver, method))
    assert solver.lib.sf_set_obstacle_maccormack.argtypes == [C.c_void_p, C.c_int]
    assert solver.lib.sf_obstacle_maccormack_get.argtypes == [C.c_void_p, C.POINTER(C.c_int)]
    assert solver.lib.sf_advect_maccormack_masked.argtypes == [C.c_void_p] + [C.c_int] * 6


def test_entry_points_reject_a_null_context_and_a_null_result():
    from fluidsolvergpu_amd import solver

    on = C.c_int(7)
    for value in (0, 1, 2):
        assert solver.lib.sf_set_obstacle_maccormack(None, value) == solver.SF_ERR_INVALID
    assert solver.lib.sf_obstacle_maccormack_get(None, C.byref(on)) == solver.SF_ERR_INVALID
    assert on.value == 7
    assert solver.lib.sf_obstacle_maccormack_get(None, None) == solver.SF_ERR_INVALID
    assert solver.lib.sf_advect_maccormack_masked(None, 0, 6, 7, 0, 1, 2) == solver.SF_ERR_INVALID


def test_driver_takes_obstacle_maccormack():
    """With --obstacle-transport the option lets every --maccormack through the option check (the run then needs a
    device: exit 0 with one, 1 without); without --obstacle-transport it is refused with a message naming both options;
    without it, --obstacle-transport --maccormack is refused as before."""
    base = ("--n", "8", "--steps", "1", "--every", "0", "--quiet")
    for which in ("vel", "dens", "both"):
        out = driver(*base, *BOX, "--obstacle-transport", "--obstacle-maccormack", "--maccormack", which)
        assert out.returncode in (0, 1), (which, out.returncode, out.stderr)
        assert "does not go with" not in out.stderr and "unknown option" not in out.stderr and "needs" not in out.stderr, out.stderr
        if out.returncode == 1:
            assert "SF_ERR_NO_DEVICE" in out.stderr, out.stderr
    out = driver(*base, *BOX, "--obstacle-transport", "--obstacle-maccormack")  # no MacCormack scheme: the setting alone
    assert out.returncode in (0, 1) and "needs" not in out.stderr, (out.returncode, out.stderr)
    for extra in ((), ("--maccormack", "both")):
        out = driver(*base, *BOX, "--obstacle-maccormack", *extra)
        assert out.returncode == 2, (out.returncode, out.stderr)
        assert "--obstacle-maccormack" in out.stderr and "--obstacle-transport" in out.stderr, out.stderr
    out = driver(*base, *BOX, "--obstacle-transport", "--maccormack", "both")
    assert out.returncode == 2 and "--obstacle-transport does not go with --maccormack" in out.stderr
    assert "--obstacle-maccormack" in driver("--help").stdout + driver("--help").stderr
