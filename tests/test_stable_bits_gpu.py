"""The SPEC §3 operators and the tracers of libsfgpu.so against the C++ oracle, bit for bit, on inputs with NaN, +-inf,
signed zeros, subnormals, values that overflow and traces that land exactly on cell centres and clamp bounds
(tests/stable_cases.py; tests/test_stable_inputs_ref.py shows on the CPU what these inputs tell apart). The comparison
is gpu_support.assert_same_bits with nan_ok: NaN payloads differ between x86 and gfx950, which entries are NaN must
not. Every case first checks on the reference that fewer than a quarter of each compared field is NaN."""
import numpy as np
import pytest

import oracle_lib as O
import shape_cases as C
import stable_cases as SC
from gpu_support import (DIFF, DT, DTYPES, NAMES, USER, VISC, advect_form, assert_same_bits, check_transport, make,  # noqa: F401
                         march_mode, upload_all)  # (advect_form, march_mode: fixtures)
from shape_cases import dname

pytestmark = pytest.mark.gpu

SHAPES = [(N, t) for N in C.SIZES for t in DTYPES]
IDS = [f"N{N}-{dname(t)}" for N, t in SHAPES]


def same(got, want, what):
    SC.check_nan_share([want], what)
    assert_same_bits(got, want, what, nan_ok=True)


def typed(cases):
    return [c + (t,) for c in cases for t in DTYPES]


def ids(cases):
    return ["-".join(dname(v) if isinstance(v, type) else str(v) for v in c) for c in cases]


# ---- add_source, set_bnd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", SHAPES, ids=IDS)
def test_add_source_and_set_bnd(N, dtype):
    with make(N, dtype) as fs:
        for family in SC.FAMILIES:
            x, s = SC.pointwise_inputs(N, dtype, family)
            fs.upload("dens", x)
            fs.upload("dens0", s)
            fs.add_source("dens", "dens0")
            want = x.copy()
            O.add_source(want, s, dtype(DT))
            same(fs.download("dens"), want, f"add_source {family}")
            for b in range(4):
                fs.upload("u", x)
                fs.set_bnd(b, "u")
                want = x.copy()
                O.set_bnd(b, want)
                same(fs.download("u"), want, f"set_bnd {family} b={b}")


# ---- lin_solve ---------------------------------------------------------------------------------------------------------
def check_lin_solve(fs, N, dtype, K, inputs, what):
    x, x0 = inputs
    for b in range(4):
        fs.upload("dens", x)
        fs.upload("dens0", x0)
        fs.lin_solve(b, "dens", "dens0", SC.A_LIN, SC.C_LIN, K)
        fs.sync()
        want = x.copy()
        O.lin_solve(b, want, x0, dtype(SC.A_LIN), dtype(SC.C_LIN), K)
        same(fs.download("dens"), want, f"{what} b={b}")
        assert_same_bits(fs.download("dens0"), x0, f"{what} b={b}: x0 must come back untouched")


LIN = typed(SC.LIN_CASES) + SC.LIN_BIG


@pytest.mark.parametrize("N,K,dtype", LIN, ids=ids(LIN))
def test_lin_solve(N, K, dtype, march_mode):
    with make(N, dtype) as fs:
        for family in SC.FAMILIES if N <= 130 else SC.FAMILIES[:1]:
            check_lin_solve(fs, N, dtype, K, SC.lin_inputs(N, dtype, family, K), f"lin_solve {family} K={K}")


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_lin_solve_non_finite_values_on_five_cells(dtype, march_mode):
    x, x0, K = SC.lin_n5_nonfinite(dtype)
    with make(5, dtype) as fs:
        check_lin_solve(fs, 5, dtype, K, (x, x0), "lin_solve N=5")


LIN_SW = typed(SC.LIN_SWITCH_CASES)


@pytest.mark.parametrize("env", SC.LIN_SWITCHES, ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("N,K,dtype", LIN_SW, ids=ids(LIN_SW))
def test_lin_solve_under_switches(N, K, dtype, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SF_MARCH_MINCELLS_K", "0")
    with make(N, dtype) as fs:
        for family in SC.FAMILIES:
            check_lin_solve(fs, N, dtype, K, SC.lin_inputs(N, dtype, family, K), f"lin_solve {env} {family} K={K}")


# ---- project -------------------------------------------------------------------------------------------------------------
PROJECT = typed(SC.PROJECT_CASES)


@pytest.mark.parametrize("N,K,dtype", PROJECT, ids=ids(PROJECT))
def test_project(N, K, dtype, march_mode, monkeypatch):
    """u, v, w and p (u0), div (v0). (64, 8) under "marching" takes the zero-iterate first pass of the marching
    kernel; K = 0 runs the two halves alone."""
    f = SC.project_inputs(N, dtype, K)
    want = {n: a.copy() for n, a in f.items()}
    O.project(want["u"], want["v"], want["w"], want["u0"], want["v0"], K)
    for skip in ("0", "1"):
        for first in ("0", "1"):
            monkeypatch.setenv("SF_ZERO_SKIP", skip)
            monkeypatch.setenv("SF_SK_FIRST", first)
            with make(N, dtype, K=K) as fs:
                upload_all(fs, f)
                fs.project("u", "v", "w", "u0", "v0")
                fs.sync()
                for n in f:
                    same(fs.download(n), want[n], f"project ZERO_SKIP={skip} SK_FIRST={first}: {n}")


# ---- advect ----------------------------------------------------------------------------------------------------------------
def check_advect(fs, dtype, inputs, dt, what):
    d0, u, v, w = inputs
    for n, a in (("dens0", d0), ("u", u), ("v", v), ("w", w)):
        fs.upload(n, a)
    for b in range(4):
        fs.advect(b, "dens", "dens0", "u", "v", "w")
        fs.sync()
        want = np.zeros_like(d0)
        O.advect(b, want, d0, u, v, w, dtype(dt))
        same(fs.download("dens"), want, f"{what} b={b}")


ADVECT = SHAPES + SC.ADVECT_BIG


@pytest.mark.parametrize("N,dtype", ADVECT, ids=ids(ADVECT))
def test_advect(N, dtype, advect_form):
    with make(N, dtype) as fs:
        check_advect(fs, dtype, SC.advect_inputs(N, dtype), DT, "advect")


LANDING = typed(SC.LANDING_CASES)


@pytest.mark.parametrize("N,dt,dtype", LANDING, ids=ids(LANDING))
def test_advect_exact_landings(N, dt, dtype, advect_form):
    with make(N, dtype) as fs:
        fs.set_coefficients(dt, DIFF, VISC)
        check_advect(fs, dtype, C.exact_landing(N, dtype, N, dt), dt, "advect, exact landings")


# ---- decomposed contexts -----------------------------------------------------------------------------------------------------
DECOMPOSED = typed(C.DECOMPOSED)


@pytest.mark.parametrize("N,P,transport,dtype", DECOMPOSED, ids=ids(DECOMPOSED))
def test_decomposed_lin_solve_and_advect(N, P, transport, dtype, advect_form):
    """Non-finite values in the solved and advected fields only; fs.sync() raises if a status is not clean."""
    K = 4
    with make(N, dtype, P=P, transport=transport) as fs:
        check_advect(fs, dtype, SC.advect_inputs(N, dtype, finite_velocity=True), DT, f"advect P={P}")
        if N <= 130 and advect_form == "default":
            check_lin_solve(fs, N, dtype, K, SC.lin_inputs(N, dtype, "specials", K), f"lin_solve P={P} K={K}")
        check_transport(fs, transport, P)


# ---- full steps ------------------------------------------------------------------------------------------------------------------
def check_steps(N, P, bound, state, dtype):
    K = SC.STEP_K
    f = SC.step_inputs(N, dtype, state)
    src = {n: f[n].copy() for n in USER}
    with make(N, dtype, K=K, P=P) as fs:
        upload_all(fs, f)
        if bound:
            for n, slot in USER.items():
                fs.upload(slot, src[n])
            fs.bind_sources(*USER.values())
        for step in range(2):
            if step and not bound:
                upload_all(fs, src)
            fs.vel_step()
            fs.dens_step()
        fs.sync()
        got = {n: fs.download(n) for n in NAMES}
    for _ in range(2):
        for n in src:
            f[n][...] = src[n]
        O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in NAMES:
        same(got[n], f[n], f"two steps {state} P={P} bound={bound}: {n}")


STEPS = typed(SC.STEP_CASES)


@pytest.mark.parametrize("N,P,bound,state,dtype", STEPS, ids=ids(STEPS))
def test_full_steps(N, P, bound, state, dtype):
    check_steps(N, P, bound, state, dtype)


def test_full_steps_graph_replay(monkeypatch):
    monkeypatch.setenv("SF_GRAPH", "1")
    check_steps(34, 1, True, "random", np.float32)


# ---- tracers -------------------------------------------------------------------------------------------------------------------------
def check_tracers(N, dtype, exact):
    pos, f, dt = SC.tracer_inputs(N, dtype, exact)
    with make(N, dtype) as fs:
        fs.set_coefficients(dt, DIFF, VISC)
        upload_all(fs, f)
        fs.tracers_set(pos)
        for _ in range(3):
            fs.tracers_advect()
        got = fs.tracers_get()
    want = pos.copy()
    for _ in range(3):
        O.tracers_advect(want, f["u"], f["v"], f["w"], dtype(dt))
    for g, w, what in zip(got, (want,) + O.tracers_sample(want, f["dens"], f["u"], f["v"], f["w"]), ("position", "density", "speed")):
        same(g, w, f"tracer {what}")


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("N", SC.TRACER_SIZES)
def test_tracers(N, dtype):
    check_tracers(N, dtype, exact=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_tracers_carried_exactly_onto_a_bound(dtype):
    check_tracers(16, dtype, exact=True)
