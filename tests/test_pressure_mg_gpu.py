"""The multigrid V-cycle preconditioner of the conjugate-gradient projection (docs/SPEC.md §11.3,
sf_set_pressure_multigrid, sf_precondition): the device must leave the bits of tests/pressure_mg_ref.py.

(a) sf_precondition against vcycle: every no-coarsening size and hierarchy shape under four settings, the second-trip
    sizes, two calls in a row, and the Jacobi kind through the same call;
(b) sf_project_cg against the reference: fields, iterations, status, rel_residual;
(c) the admissible decompositions (sf_precondition and six iterations each) and the rejected ones;
(d) check_every in {0, 1, 4}, a zero right-hand side, a NaN in the velocity;
(e) two vel_step with CG and multigrid against the step composed in numpy, under three switch settings;
(f) the settings: getter, the Jacobi setting kept and restored, no mg_ op on a context that never enabled multigrid.
tests/test_pressure_mg_ref.py shows on the CPU which wrong V-cycle these inputs tell from the right one. The
schedule-hazard check of tests/conftest.py reads the trace of every context created here."""
import os
import time

import numpy as np
import pytest

import diagnostics_ref as D
import mg_cases as MC
import pressure_cg_ref as R
import pressure_mg_ref as G
import pressure_pcg_ref as Q
import shape_cases as C
from gpu_support import S, assert_same_bits, check_solve, make, random_fields, slab0_ops, upload_all

pytestmark = pytest.mark.gpu

I = R.I
TOL = MC.TOL
OUT = (("u", "u"), ("v", "v"), ("w", "w"), ("u0", "p"), ("v0", "div"))
_VCYCLES, _SOLVES = {}, {}


def want_vcycle(N, dtype, s):
    """vcycle of the case's right-hand side: computed once, only read afterwards."""
    key = (N, C.dname(dtype), s)
    if key not in _VCYCLES:
        t0 = time.perf_counter()
        _, r = MC.precondition_fields(N, dtype)
        _VCYCLES[key] = G.vcycle(r[I, I, I], *s)
        print(f"vcycle {key}: {time.perf_counter() - t0:.1f} s")
    return _VCYCLES[key]


def want_solve(N, dtype, max_iters, s):
    key = (N, C.dname(dtype), max_iters, s)
    if key not in _SOLVES:
        t0 = time.perf_counter()
        _SOLVES[key] = G.project_cg(*C.cg_velocity(N, dtype, C.cg_seed(N)), TOL, max_iters, *s)
        print(f"project_cg {key}: {time.perf_counter() - t0:.1f} s")
    return _SOLVES[key]


def multigrid(fs, s):
    fs.set_pressure_multigrid(*s)
    got = fs.pressure_multigrid
    assert (got["sweeps"], got["max_levels"], got["coarse_sweeps"]) == s
    return got


def check_precondition(fs, N, dtype, s, what, calls=2):
    """z and r uploaded with independent random shells; z = M(r) whole against the reference, `calls` times."""
    z0, r = MC.precondition_fields(N, dtype)
    want = want_vcycle(N, dtype, s)
    fs.upload("u0", z0)
    fs.upload("v0", r)
    for n in range(calls):
        fs.precondition("u0", "v0")
        fs.sync()
        assert_same_bits(fs.download("u0"), want, f"{what}: call {n}")
    assert_same_bits(fs.download("v0"), r, f"{what}: r is left alone")


# ---- (a) -----------------------------------------------------------------------------------------------------------
SHAPES = [(N, t) for N in MC.SIZES for t in C.DTYPES]


@pytest.mark.parametrize("s", MC.SETTINGS, ids=MC.setting_id)
@pytest.mark.parametrize("N,dtype", SHAPES, ids=[f"N{n}-{C.dname(t)}" for n, t in SHAPES])
def test_precondition(N, dtype, s):
    """Sizes that do not coarsen (the cycle is nu_c sweeps on the fine grid) and every shape of hierarchy; (1, 0, 1): the
    first sweep alone on every level; (3, 2, 4) and (2, 1, 8): capped hierarchies. Two calls in a row: the second starts
    from the first one's z."""
    with make(N, dtype) as fs:
        got = multigrid(fs, s)
        assert got["levels"] == len(G.levels(N, s[1]))
        check_precondition(fs, N, dtype, s, MC.case_id(N, dtype, s))


@pytest.mark.parametrize("N,dtype", MC.SECOND_TRIP, ids=[f"N{n}-{C.dname(t)}" for n, t in MC.SECOND_TRIP])
def test_precondition_where_a_fine_row_takes_a_second_trip(N, dtype):
    """More than 64 vectors per fine row: the restriction's pairs and the prolongation's parents of the second trip
    (264 -> 132 -> 66 -> 33: a second trip on two levels in fp32)."""
    assert C.second_trip(N, dtype)
    with make(N, dtype) as fs:
        multigrid(fs, MC.DEFAULT)
        check_precondition(fs, N, dtype, MC.DEFAULT, MC.case_id(N, dtype), calls=1)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
@pytest.mark.parametrize("N,m", [(13, 3), (34, 4), (34, 1)], ids=["N13-m3", "N34-m4", "N34-m1"])
def test_precondition_with_the_jacobi_kind(N, m, dtype):
    """sf_precondition with SF_PRECOND_JACOBI in force is lin_solve(0, z, r, 1, 6, m) from zero."""
    z0, r = MC.precondition_fields(N, dtype)
    want = Q.precondition(r[I, I, I], m)
    with make(N, dtype) as fs:
        fs.set_pressure_preconditioner("jacobi", m)
        fs.upload("u0", z0)
        fs.upload("v0", r)
        for n in range(2):
            fs.precondition("u0", "v0")
            fs.sync()
            assert_same_bits(fs.download("u0"), want, f"jacobi:{m} N={N} call {n}")


def test_precondition_refuses_when_nothing_is_in_force():
    with make(8, np.float32) as fs:
        for z, r in (("u0", "v0"), ("u0", "u0")):
            with pytest.raises(S().SfError) as e:
                fs.precondition(z, r)
            assert e.value.status == S().SF_ERR_INVALID
        multigrid(fs, MC.DEFAULT)
        with pytest.raises(S().SfError) as e:
            fs.precondition("u0", "u0")
        assert e.value.status == S().SF_ERR_INVALID
        check_precondition(fs, 8, np.float32, MC.DEFAULT, "after the refusals")


# ---- (b) -----------------------------------------------------------------------------------------------------------
SOLVES = [(N, t) for N in MC.SOLVE_SIZES for t in C.DTYPES]


@pytest.mark.parametrize("N,dtype", SOLVES, ids=[f"N{n}-{C.dname(t)}" for n, t in SOLVES])
def test_project_cg_to_convergence(N, dtype):
    """(2, 0, 8) on the random velocity, to convergence. N = 1: r = 0 and no iteration; the reference decides."""
    want = want_solve(N, dtype, MC.TO_CONVERGENCE, MC.DEFAULT)
    assert want["status"] == R.CONVERGED and (want["iterations"] == 0) == (N == 1)
    with make(N, dtype) as fs:
        multigrid(fs, MC.DEFAULT)
        check_solve(fs, *C.cg_velocity(N, dtype, C.cg_seed(N)), TOL, MC.TO_CONVERGENCE, f"N={N} {C.dname(dtype)}", want=want)


@pytest.mark.parametrize("N,dtype", MC.LONG_SOLVES, ids=[f"N{n}-{C.dname(t)}" for n, t in MC.LONG_SOLVES])
def test_project_cg_two_iterations_at_the_second_trip_sizes(N, dtype):
    want = want_solve(N, dtype, MC.LONG_ITERS, MC.DEFAULT)
    assert (want["status"], want["iterations"]) == (R.MAX_ITERS, MC.LONG_ITERS)
    with make(N, dtype) as fs:
        multigrid(fs, MC.DEFAULT)
        check_solve(fs, *C.cg_velocity(N, dtype, C.cg_seed(N)), TOL, MC.LONG_ITERS, f"N={N} {C.dname(dtype)}", want=want)


# ---- (c) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
@pytest.mark.parametrize("N,P,transport,L", MC.DECOMPOSED, ids=[f"N{n}-P{p}-{tr}-L{l}" for n, p, tr, l in MC.DECOMPOSED])
def test_every_admissible_decomposition(N, P, transport, L, dtype):
    """The bits of the P = 1 reference: the ghost planes of z travel after every sweep and after the correction on every
    level, no restriction crosses a slab, gamma's plane records cross the slabs. Scalars on the host and on the device."""
    s = (2, L, 8)
    want = want_solve(N, dtype, MC.DECOMPOSED_ITERS, s)
    with make(N, dtype, P=P, transport=transport) as fs:
        got = multigrid(fs, s)
        assert got["levels"] == len(G.levels(N, L))
        check_precondition(fs, N, dtype, s, MC.case_id(N, dtype, s, P))
        for every in (0, 4):
            fs.set_pressure_sync(every)
            check_solve(fs, *C.cg_velocity(N, dtype, C.cg_seed(N)), TOL, MC.DECOMPOSED_ITERS,
                        f"N={N} P={P} {transport} {s} sync={every}", want=want)
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


@pytest.mark.parametrize("N,P,deepest", MC.REJECTED, ids=[f"N{n}-P{p}" for n, p, _ in MC.REJECTED])
def test_inadmissible_decompositions_are_rejected(N, P, deepest):
    with make(N, np.float32, P=P) as fs:
        multigrid(fs, (1, deepest, 3))
        before = fs.pressure_multigrid
        for max_levels in (0, deepest + 1):
            with pytest.raises(S().SfError) as e:
                fs.set_pressure_multigrid(2, max_levels, 8)
            assert e.value.status == S().SF_ERR_INVALID
            assert f"max_levels is {deepest}" in str(e.value), str(e.value)
            assert fs.pressure_multigrid == before
        multigrid(fs, (2, deepest, 8))
        multigrid(fs, (0, 0, 8))  # off: the depth is kept, not used, and not checked


# ---- (d) -----------------------------------------------------------------------------------------------------------
STOP_N = 24


def stop_inputs():
    out = {}
    for dtype in C.DTYPES:
        t = C.dname(dtype)
        u, v, w = C.cg_velocity(STOP_N, dtype, 7)
        out[f"converges-{t}"] = (u, v, w, 1e-3, 100)
        out[f"max_iters3-{t}"] = (u, v, w, 1e-6, 3)
        z = np.zeros_like(u)
        out[f"zero-{t}"] = (z, z.copy(), z.copy(), 1e-3, 10)
        bad = v.copy()
        bad[5, 6, 7] = np.nan
        out[f"nan-{t}"] = (u, bad, w, 1e-3, 10)
    return out


STOP = stop_inputs()


@pytest.mark.parametrize("P", [1, 3], ids=["P1", "P3"])
@pytest.mark.parametrize("name", list(STOP))
def test_check_every_leaves_the_same_bits(name, P):
    """check_every in {0, 1, 4} on one context, each against the reference: the V-cycles of iterations enqueued past the
    stop run and change nothing a result reads. Zero right-hand side: CONVERGED, 0 iterations. NaN: BREAKDOWN, and
    sf_sync stays SF_OK (the context solves the next input)."""
    u, v, w, tol, max_iters = STOP[name]
    dtype = u.dtype.type
    want = G.project_cg(u, v, w, tol, max_iters, *MC.DEFAULT)
    if name.startswith("converges"):
        assert want["status"] == R.CONVERGED and want["iterations"] % 4
    if name.startswith("max_iters3"):
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, 3)
    if name.startswith("zero"):
        assert (want["status"], want["iterations"]) == (R.CONVERGED, 0)
    if name.startswith("nan"):
        assert (want["status"], want["iterations"]) == (R.BREAKDOWN, 0)
    with make(STOP_N, dtype, P=P, transport="rccl-self" if dtype == np.float32 else "copy") as fs:
        multigrid(fs, MC.DEFAULT)
        for every in (0, 1, 4):
            fs.set_pressure_sync(every)
            what = f"{name} P={P} check_every={every}"
            if name.startswith("nan"):
                for n, a in (("u", u), ("v", v), ("w", w)):
                    fs.upload(n, a)
                info = fs.project_cg("u", "v", "w", "u0", "v0", tol, max_iters)
                fs.sync()  # SF_OK: raises otherwise
                assert (info["status"], info["iterations"]) == (R.BREAKDOWN, 0), what
                assert np.isnan(info["rel_residual"]) and np.isnan(want["rel_residual"]), what
                for slot, n in OUT:
                    assert_same_bits(fs.download(slot), want[n], f"{what}: {n}", nan_ok=True)
            else:
                check_solve(fs, u, v, w, tol, max_iters, what, want=want)
        if name.startswith("nan"):
            vel = C.cg_velocity(STOP_N, dtype, 5)
            check_solve(fs, *vel, TOL, 6, "the next solve on the context", want=G.project_cg(*vel, TOL, 6, *MC.DEFAULT))


# ---- (e) -----------------------------------------------------------------------------------------------------------
_STEPS = {}
STEP_SETTINGS = [{}, {"SF_ISHELL": "0"}, {"SF_MARCH_MINCELLS_K": "0"}]


@pytest.mark.parametrize("env", STEP_SETTINGS, ids=["default", "ishell0", "marching"])
@pytest.mark.parametrize("P,L", [(1, 0), (4, 2)], ids=["P1", "P4-L2"])
def test_vel_step_with_multigrid(P, L, env, monkeypatch):
    """Two vel_step at N = 40 fp32 with CG (1e-2, 10) and the V-cycle (2, L, 8), the sources uploaded again in between."""
    N, dtype, K, tol, max_iters = 40, np.float32, 6, 1e-2, 10
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = (2, L, 8)
    f = random_fields(N, dtype, 41)
    if s not in _STEPS:
        g, outs = dict(f), []
        for _ in range(2):
            out = MC.reference_vel_step(g, K, tol, max_iters, s)
            outs.append(out)
            g = dict(f, u=out["u"], v=out["v"], w=out["w"])
        _STEPS[s] = outs
    outs = _STEPS[s]
    assert all(o["iterations"] >= 1 for o in outs)
    with make(N, dtype, K=K, P=P) as fs:
        upload_all(fs, f)
        fs.set_pressure_solver("cg", tol, max_iters)
        multigrid(fs, s)
        for step, out in enumerate(outs):
            fs.vel_step()
            info = fs.pressure_info()
            print(f"P={P} step {step}: {info}")
            assert (info["solver"], info["status"], info["iterations"]) == (S().SF_PRESSURE_CG, out["status"], out["iterations"])
            assert D.bits(info["rel_residual"]) == D.bits(out["rel_residual"])
            for n in ("u", "v", "w"):
                assert_same_bits(fs.download(n), out[n], f"P={P} step {step}: {n}")
            for n in ("u0", "v0", "w0"):
                fs.upload(n, f[n])


# ---- (f) -----------------------------------------------------------------------------------------------------------
def test_settings_are_kept_and_the_jacobi_solve_comes_back():
    N, dtype = 34, np.float64
    u, v, w = C.cg_velocity(N, dtype, C.cg_seed(N))
    jac = {"kind": S().SF_PRECOND_JACOBI, "sweeps": 4}
    with make(N, dtype) as fs:
        assert fs.pressure_multigrid == {"sweeps": 0, "max_levels": 0, "coarse_sweeps": 8, "levels": 2}
        fs.set_pressure_preconditioner("jacobi", 4)
        jacobi = check_solve(fs, u, v, w, TOL, 8, "jacobi:4", want=Q.project_cg(u, v, w, TOL, 8, 4))
        fs.set_pressure_multigrid(3, 1, 5)
        assert fs.pressure_multigrid == {"sweeps": 3, "max_levels": 1, "coarse_sweeps": 5, "levels": 1}
        fs.set_pressure_multigrid(2)
        assert fs.pressure_multigrid == {"sweeps": 2, "max_levels": 0, "coarse_sweeps": 8, "levels": 2}
        assert fs.pressure_preconditioner == jac  # kept and reported, not used
        check_solve(fs, u, v, w, TOL, 8, "multigrid over jacobi:4", want=want_solve(N, dtype, 8, MC.DEFAULT))
        assert fs.pressure_sync["host_waits"] == 3 + 3 * want_solve(N, dtype, 8, MC.DEFAULT)["iterations"] - (
            1 if want_solve(N, dtype, 8, MC.DEFAULT)["status"] == R.CONVERGED else 0)
        for bad in ((-1, 0, 8), (2, -1, 8), (2, 0, 0), (0, 0, 0)):
            with pytest.raises(S().SfError) as e:
                fs.set_pressure_multigrid(*bad)
            assert e.value.status == S().SF_ERR_INVALID
        assert fs.pressure_multigrid == {"sweeps": 2, "max_levels": 0, "coarse_sweeps": 8, "levels": 2}
        fs.set_pressure_multigrid(0, 3, 2)
        assert fs.pressure_multigrid == {"sweeps": 0, "max_levels": 3, "coarse_sweeps": 2, "levels": 2}
        assert fs.pressure_preconditioner == jac
        check_solve(fs, u, v, w, TOL, 8, "jacobi:4 again", want=jacobi)


def test_a_context_without_multigrid_issues_no_mg_op():
    N, dtype = 16, np.float32
    u, v, w = C.cg_velocity(N, dtype, C.cg_seed(N))
    path = os.environ["SF_TRACE_SCHEDULE"]
    with make(N, dtype) as fs:
        fs.set_pressure_preconditioner("jacobi", 4)
        check_solve(fs, u, v, w, TOL, 6, "jacobi:4", want=Q.project_cg(u, v, w, TOL, 6, 4))
        names = [op["name"] for op in slab0_ops(path)]
        assert "cg_dot" in names and not [n for n in names if n.startswith("mg_")]
        multigrid(fs, MC.DEFAULT)
        check_solve(fs, u, v, w, TOL, 6, "multigrid", want=want_solve(N, dtype, 6, MC.DEFAULT))
        names = [op["name"] for op in slab0_ops(path)]
        assert {"mg_smooth0", "mg_smooth", "mg_restrict", "mg_prolong"} <= set(names)
