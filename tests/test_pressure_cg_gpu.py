"""The conjugate-gradient projection on the GPU (docs/SPEC.md §11): sf_project_cg, sf_poisson_residual, the pressure
solver of vel_step and sf_pressure_info_get through libsfgpu.so against the numpy reference (tests/pressure_cg_ref.py).
Every comparison is exact equality of bits — fields on all stored cells, iteration counts, status, residuals — for every
decomposition and transport of the case table. The schedule-hazard checker of tests/conftest.py sees every new launch."""
import math

import numpy as np
import pytest

import diagnostics_ref as D
import pressure_cg_ref as R
from gpu_support import (DTYPE_IDS, DTYPES, OPERATOR_CASES, VISC, S, assert_same_bits, check_solve, make, random_fields,
                         upload_all)
from shape_cases import cg_velocity as random_velocity

pytestmark = pytest.mark.gpu

CASES = sorted(OPERATOR_CASES + [(32, 1, "copy"), (32, 4, "copy")])
CASE_IDS = [f"N{n}-P{p}-{t}" for n, p, t in CASES]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N,P,transport", CASES, ids=CASE_IDS)
def test_project_cg_matches_the_reference(N, P, transport, dtype):
    """A random velocity (shells as uploaded: the operator reads neighbours as stored) stopped by max_iters, and the
    smooth field of §11 run to convergence."""
    with make(N, dtype, P=P, transport=transport) as fs:
        g0 = fs.transport_info()["rccl_groups"]
        want = check_solve(fs, *random_velocity(N, dtype, 500 + N + P), 1e-3, 8, f"random N={N} P={P} {transport}")
        assert want["status"] == R.MAX_ITERS
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > g0
        want = check_solve(fs, *R.smooth_velocity(N, dtype), 1e-3, 64, f"smooth N={N} P={P} {transport}")
        assert want["status"] == R.CONVERGED
        info = fs.pressure_info()
        assert info["solves_total"] == 2 and info["iterations_total"] == 8 + want["iterations"]


@pytest.mark.parametrize("N,dtype", [(1, np.float32), (2, np.float32), (3, np.float32), (130, np.float32), (260, np.float32),
                                     (1, np.float64), (2, np.float64), (3, np.float64), (130, np.float64)],
                         ids=lambda x: str(x) if isinstance(x, int) else x.__name__)
def test_small_ragged_and_two_trip_rows(N, dtype):
    """N = 1, 2, 3 (every cell a wall cell), 130 (ragged vectors; the second trip of an fp64 row) and 260 fp32 (the
    second trip of an fp32 row), at max_iters = 8. At 130 fp64 and 260 fp32 the second trip is lane 0's single vector:
    neither the order of a second trip's additions nor lane_up / lane_dn inside the second stretch can show there.
    tests/test_pressure_cg_shapes_gpu.py runs the sizes that do (N = 64 W, 64 W + 1, 131 / 262, 200 / 324)."""
    with make(N, dtype) as fs:
        check_solve(fs, *random_velocity(N, dtype, 600 + N), 1e-3, 8, f"N={N}")


@pytest.mark.parametrize("N,P", [(130, 2), (130, 5)])
def test_ragged_rows_decomposed(N, P):
    with make(N, np.float64, P=P) as fs:
        check_solve(fs, *random_velocity(N, np.float64, 700 + P), 1e-3, 4, f"N={N} P={P}")


def test_bench_size_256():
    N, dtype = 256, np.float32
    with make(N, dtype) as fs:
        check_solve(fs, *R.smooth_velocity(N, dtype), 1e-3, 12, "256^3")


@pytest.mark.parametrize("P,transport", [(1, "copy"), (4, "copy"), (2, "rccl-self")])
def test_residual_after_both_solvers_and_the_motivation(P, transport):
    """N = 64 fp32, the smooth field: sf_poisson_residual equals the reference's bits after sf_project (Jacobi, K = 20)
    and after sf_project_cg; Jacobi leaves >= 0.5 of the right-hand side, CG at tol = 1e-3 at most 4 tol."""
    N, dtype, tol = 64, np.float32, 1e-3
    u, v, w = R.smooth_velocity(N, dtype)
    with make(N, dtype, K=20, P=P, transport=transport) as fs:
        for n, a in (("u", u), ("v", v), ("w", w)):
            fs.upload(n, a)
        fs.project("u", "v", "w", "u0", "v0")
        res_j = fs.poisson_residual("u0", "v0")
        jac = R.project_jacobi(u, v, w, 20)
        assert_same_bits(fs.download("u0"), jac["p"], "jacobi p")
        assert D.bits(res_j) == D.bits(R.poisson_residual(jac["p"], jac["div"]))
        info = fs.pressure_info()
        assert (info["solver"], info["status"], info["iterations"]) == (S().SF_PRESSURE_JACOBI, S().SF_CG_MAX_ITERS, 20)
        want = check_solve(fs, u, v, w, tol, 64, f"P={P} {transport}")
        res_c = fs.poisson_residual("u0", "v0")
        print(f"jacobi K=20 residual {res_j!r}; cg iterations {want['iterations']} residual {res_c!r}")
        assert res_j >= 0.5
        assert want["status"] == R.CONVERGED and res_c <= 4 * tol
        assert fs.poisson_residual("user0", "user1") == 0.0  # zero div


def composed_step(fs, forces, mc, tol, max_iters):
    """SPEC §3 vel_step (with §8 forces and §9 advection when asked for) from the single operators of the C ABI, its two
    projections being sf_project_cg. The ABI has no swap: the slots change roles instead."""
    if forces:
        fs.add_forces("u", "v", "w", "dens", "u0", "v0", "w0")
    for x, s in (("u", "u0"), ("v", "v0"), ("w", "w0")):
        fs.add_source(x, s)
    for b, x, s in ((1, "u0", "u"), (2, "v0", "v"), (3, "w0", "w")):  # swapped: the sources are the initial iterate
        fs.diffuse(b, x, s, VISC)
    first = fs.project_cg("u0", "v0", "w0", "u", "v", tol, max_iters)
    adv = fs.advect_maccormack if mc else fs.advect
    for b, d, d0 in ((1, "u", "u0"), (2, "v", "v0"), (3, "w", "w0")):
        adv(b, d, d0, "u0", "v0", "w0")
    second = fs.project_cg("u", "v", "w", "u0", "v0", tol, max_iters)
    return first, second


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("forces_mc", [False, True], ids=["plain", "forces-maccormack"])
def test_vel_step_with_cg_is_the_composed_step(forces_mc, P, dtype):
    vel_step_against_the_composed_step(forces_mc, P, dtype, 6)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("forces_mc", [False, True], ids=["plain", "forces-maccormack"])
def test_vel_step_with_cg_is_the_composed_step_after_a_marching_diffuse(forces_mc, P, dtype, monkeypatch):
    """K = 9 under SF_MARCH_MINCELLS_K=0: the diffusion of vel_step runs the marching kernel, whose first pass leaves
    the i-shell of the velocity unwritten, and project_cg mirrors u's itself; the single operators write every shell."""
    monkeypatch.setenv("SF_MARCH_MINCELLS_K", "0")
    vel_step_against_the_composed_step(forces_mc, P, dtype, 9)


def vel_step_against_the_composed_step(forces_mc, P, dtype, K):
    N, tol, max_iters, steps = 32, 1e-2, 10, 2
    f = random_fields(N, dtype, 31 + P)
    out = []
    for composed in (False, True):
        with make(N, dtype, K=K, P=P) as fs:
            upload_all(fs, f)
            if forces_mc:
                fs.set_vorticity_confinement(0.3)
                fs.set_buoyancy(0.5, 0.1, 1)
                fs.set_advection(S().SF_ADVECT_MACCORMACK, S().SF_ADVECT_SEMI_LAGRANGIAN)
            infos = []
            for _ in range(steps):
                if composed:
                    infos.append(composed_step(fs, forces_mc, forces_mc, tol, max_iters)[1])
                else:
                    fs.set_pressure_solver("cg", tol, max_iters)
                    fs.vel_step()
                    infos.append(fs.pressure_info())
                for n in ("u0", "v0", "w0"):  # the sources of the next step
                    fs.upload(n, f[n])
            fs.sync()
            total = fs.pressure_info()
            assert total["solves_total"] == 2 * steps
            out.append(({n: fs.download(n) for n in ("u", "v", "w")}, infos, total["iterations_total"]))
    for n in ("u", "v", "w"):
        assert_same_bits(out[0][0][n], out[1][0][n], f"{n}: vel_step with CG against the composed step")
    assert out[0][2] == out[1][2]
    for a, b in zip(out[0][1], out[1][1]):  # sf_pressure_info_get reports the second projection of the step
        assert (a["solver"], a["status"], a["iterations"]) == (b["solver"], b["status"], b["iterations"])
        assert D.bits(a["rel_residual"]) == D.bits(b["rel_residual"])
        assert a["solver"] == S().SF_PRESSURE_CG


@pytest.mark.parametrize("P", [1, 4])
def test_set_back_to_jacobi_is_the_untouched_context(P):
    N, dtype = 32, np.float32
    f = random_fields(N, dtype, 77)
    out = []
    for touched in (False, True):
        with make(N, dtype, K=6, P=P) as fs:
            upload_all(fs, f)
            if touched:
                fs.set_pressure_solver("cg", 1e-2, 5)
                fs.set_pressure_solver("jacobi", 1e-2, 5)
            for _ in range(2):
                fs.vel_step()
                fs.dens_step()
            fs.sync()
            out.append({n: fs.download(n) for n in S().FIELD_NAMES})
            info = fs.pressure_info()
            assert (info["solver"], info["iterations"], info["solves_total"]) == (S().SF_PRESSURE_JACOBI, 6, 4)
    for n in S().FIELD_NAMES:
        assert_same_bits(out[1][n], out[0][n], f"{n}: Jacobi selected again against the default context")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("P", [1, 2])
def test_nan_and_no_iterations_are_statuses_not_errors(P, dtype):
    N = 24
    u, v, w = R.smooth_velocity(N, dtype)
    with make(N, dtype, P=P) as fs:
        want = check_solve(fs, u, v, w, 1e-3, 0, "max_iters = 0")
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, 0)
        assert_same_bits(fs.download("u"), u, "u after no iteration")  # p = 0: u - c_grad*(0 - 0)
        bad = u.copy()
        bad[N // 2, 3, 5] = np.nan
        for n, a in (("u", bad), ("v", v), ("w", w)):
            fs.upload(n, a)
        info = fs.project_cg("u", "v", "w", "u0", "v0", 1e-3, 20)
        fs.sync()  # SF_OK: a breakdown is a status
        ref = R.project_cg(bad, v, w, 1e-3, 20)
        assert info["status"] == ref["status"] == R.BREAKDOWN
        assert info["iterations"] == ref["iterations"] and info["iterations"] in (0, 1)
        assert math.isnan(info["rel_residual"])
        assert np.array_equal(np.isnan(fs.download("u")), np.isnan(ref["u"]))
        check_solve(fs, u, v, w, 1e-3, 30, "the context works afterwards")


def test_invalid_arguments():
    import ctypes as C

    sv = S()
    with make(16, np.float32) as fs:
        for args in ((2, 1e-3, 10), (-1, 1e-3, 10), (1, 0.0, 10), (1, -1e-3, 10), (1, float("nan"), 10),
                     (1, float("inf"), 10), (1, 1e-3, -1), (0, 0.0, 10)):
            assert sv.lib.sf_set_pressure_solver(fs._h, *args) == sv.SF_ERR_INVALID, args
        for slots in ((0, 1, 2, 3, 3), (0, 0, 2, 3, 4), (0, 1, 2, 3, 12), (-1, 1, 2, 3, 4)):
            assert sv.lib.sf_project_cg(fs._h, *slots, 1e-3, 10) == sv.SF_ERR_INVALID, slots
        assert sv.lib.sf_project_cg(fs._h, 0, 1, 2, 3, 4, 0.0, 10) == sv.SF_ERR_INVALID
        assert sv.lib.sf_project_cg(fs._h, 0, 1, 2, 3, 4, 1e-3, -1) == sv.SF_ERR_INVALID
        assert sv.lib.sf_poisson_residual(fs._h, 3, 4, None) == sv.SF_ERR_INVALID
        assert sv.lib.sf_poisson_residual(fs._h, 3, 3, C.byref(C.c_double())) == sv.SF_ERR_INVALID
        assert sv.lib.sf_pressure_info_get(fs._h, None) == sv.SF_ERR_INVALID
        check_solve(fs, *R.smooth_velocity(16, np.float32), 1e-3, 30, "after the rejected calls")


def test_driver_monitor_reports_the_solve(tmp_path):
    import os
    import re
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluidsolvergpu_amd", "sf_driver")
    run = subprocess.run([exe, "--n", "32", "--steps", "4", "--monitor", "2", "--every", "0", "--quiet", "--pressure",
                          "cg:1e-2:40"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("pressure ")]
    print("\n".join(lines))
    assert len(lines) == 2
    for ln in lines:
        m = re.fullmatch(r"pressure step=(\d+) solver=cg status=(\w+) iterations=(\d+) rel_residual=(\S+) "
                         r"iterations_total=(\d+)", ln)
        assert m, ln
        assert m.group(2) == "converged" and 1 <= int(m.group(3)) <= 40 and float(m.group(4)) <= 1e-2
