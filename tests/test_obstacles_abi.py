"""CPU side of sf_set_obstacles / sf_obstacles_get (docs/SPEC.md §15): declared, exported, wrapped, the struct as the
header has it, and the driver's --obstacle parsed, and refused, before the device is touched. No GPU needed."""
import ctypes as C
import os
import subprocess

from abi_header import ROOT, declared_functions, header_text, struct_members

SYMBOLS = ("sf_set_obstacles", "sf_obstacles_get")
EXE = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")


def driver(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def test_symbols_declared_exported_and_wrapped():
    from fluidsolvergpu_amd import solver

    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in solver.ABI_SYMBOLS
        assert hasattr(solver.lib, name), f"libsfgpu.so does not export {name}"
    assert callable(solver.FluidSolver.set_obstacles) and callable(solver.FluidSolver.obstacles)
    assert solver.lib.sf_set_obstacles.argtypes == [C.c_void_p, C.c_int]
    assert solver.lib.sf_obstacles_get.argtypes == [C.c_void_p, C.POINTER(solver.SfObstacles)]


def test_struct_matches_the_header():
    from fluidsolvergpu_amd import solver

    members = struct_members(header_text(), "sf_obstacles")
    assert members == [("enabled", "int"), ("fluid_cells", "long long")]
    assert list(solver.SfObstacles._fields_) == [("enabled", C.c_int), ("fluid_cells", C.c_longlong)]
    assert C.sizeof(solver.SfObstacles) == 16
    # the table of SF_* switches and the field slots stay as they are
    assert "SF_NUM_FIELDS = 12" in header_text()


def test_entry_points_reject_a_null_context_and_a_null_result():
    from fluidsolvergpu_amd import solver

    out = solver.SfObstacles()
    assert solver.lib.sf_set_obstacles(None, 0) == solver.SF_ERR_INVALID
    assert solver.lib.sf_set_obstacles(None, -1) == solver.SF_ERR_INVALID
    assert solver.lib.sf_obstacles_get(None, C.byref(out)) == solver.SF_ERR_INVALID


GOOD = ("box:1,1,1:2,2,2", "box:3,4,5:3,4,5", "box:-2,0,1:70,9,9", "sphere:8,8,8:3", "sphere:8.5,7.25,-1:0", "sphere:1e1,2,3:2.5")
BAD = ("", "box", "box:", "box:1,2,3", "box:1,2:3,4,5", "box:1,2,3:4,5", "box:1,2,3:4,5,6:7", "box:5,5,5:4,6,6",
       "box:1,1,1:2,2,2.5", "box:1,1,x:2,2,2", "box:1,,1:2,2,2", "sphere:1,2,3", "sphere:1,2,3:", "sphere:1,2,3:-1",
       "sphere:1,2:3", "sphere:1,2,3,4:5", "sphere:1,2,3:nan", "sphere:inf,2,3:1", "blob:1,1,1:2", "1,1,1:2,2,2")


def test_driver_parses_obstacle_before_the_device():
    for spec in GOOD:
        out = driver("--pressure", "cg", "--obstacle", spec, "--bogus")
        assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (spec, out.returncode, out.stderr)
    for spec in BAD:
        out = driver("--pressure", "cg", "--obstacle", spec)
        assert out.returncode == 2 and "--obstacle takes" in out.stderr, (spec, out.returncode, out.stderr)


def test_driver_refuses_obstacles_without_cg_with_multigrid_and_more_than_sixteen():
    for args in (("--obstacle", GOOD[0]), ("--pressure", "jacobi", "--obstacle", GOOD[0]),
                 ("--obstacle", GOOD[0], "--pressure", "cg", "--pressure-mg", "2")):
        out = driver(*args)
        assert out.returncode == 2 and "--obstacle needs --pressure cg" in out.stderr, (args, out.returncode, out.stderr)
    many = [a for _ in range(16) for a in ("--obstacle", GOOD[3])]
    out = driver("--pressure", "cg", *many, "--bogus")
    assert out.returncode == 2 and "unknown option --bogus" in out.stderr, out.stderr
    out = driver("--pressure", "cg", *many, "--obstacle", GOOD[0])
    assert out.returncode == 2 and "16 times at most" in out.stderr, out.stderr
