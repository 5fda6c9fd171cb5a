"""CPU side of sf_set_obstacle_velocity / sf_obstacle_velocity_get (docs/SPEC.md §19): declared, exported, wrapped, null
contexts and a null result pointer rejected, and the driver's --obstacle-velocity with its outcomes before the device is
touched. No GPU needed."""
import ctypes as C
import os
import subprocess

from abi_header import ROOT, declared_functions

SYMBOLS = ("sf_set_obstacle_velocity", "sf_obstacle_velocity_get")
EXE = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
BOX = ("--obstacle", "box:3,3,3:5,5,5", "--pressure", "cg")
BASE = ("--n", "8", "--steps", "1", "--every", "0", "--quiet")


def driver(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    for method in ("set_obstacle_velocity", "obstacle_velocity"):
        assert callable(getattr(solver.FluidSolver, method))
    assert solver.lib.sf_set_obstacle_velocity.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int]
    assert solver.lib.sf_obstacle_velocity_get.argtypes == [C.c_void_p, C.POINTER(C.c_int)]


def test_entry_points_reject_a_null_context_and_a_null_result():
    from fluidsolvergpu_amd import solver

    on = C.c_int(7)
    for slots in ((-1, -1, -1), (8, 9, 10), (8, 8, 9)):
        assert solver.lib.sf_set_obstacle_velocity(None, *slots) == solver.SF_ERR_INVALID
    assert solver.lib.sf_obstacle_velocity_get(None, C.byref(on)) == solver.SF_ERR_INVALID
    assert on.value == 7
    assert solver.lib.sf_obstacle_velocity_get(None, None) == solver.SF_ERR_INVALID


def test_driver_takes_obstacle_velocity():
    """With --obstacle-transport the option passes the option check (the run then needs a device: exit 0 with one, 1
    without); without --obstacle-transport, with --maccormack vel or both, or with a malformed value it is refused with
    a message naming the options."""
    for extra in ((), ("--obstacle-maccormack", "--maccormack", "dens")):
        out = driver(*BASE, *BOX, "--obstacle-transport", "--obstacle-velocity", "0.5,0,-0.25", *extra)
        assert out.returncode in (0, 1), (out.returncode, out.stderr)
        assert "does not go with" not in out.stderr and "unknown option" not in out.stderr and "needs" not in out.stderr, out.stderr
        if out.returncode == 1:
            assert "SF_ERR_NO_DEVICE" in out.stderr, out.stderr
    out = driver(*BASE, *BOX, "--obstacle-velocity", "0.5,0,0")
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--obstacle-velocity" in out.stderr and "--obstacle-transport" in out.stderr, out.stderr
    for which in ("vel", "both"):
        out = driver(*BASE, *BOX, "--obstacle-transport", "--obstacle-maccormack", "--obstacle-velocity", "0.5,0,0",
                     "--maccormack", which)
        assert out.returncode == 2, (which, out.returncode, out.stderr)
        assert "--obstacle-velocity" in out.stderr and "--maccormack" in out.stderr, out.stderr
    for bad in ("1,2", "a,b,c", "1,2,nan"):
        out = driver(*BASE, *BOX, "--obstacle-transport", "--obstacle-velocity", bad)
        assert out.returncode == 2 and "--obstacle-velocity takes" in out.stderr, (bad, out.returncode, out.stderr)
    assert "--obstacle-velocity" in driver("--help").stdout + driver("--help").stderr
