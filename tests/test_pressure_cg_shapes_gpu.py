"""The conjugate-gradient projection (docs/SPEC.md §11) at every row shape, on stored shells and under the switches —
what tests/test_pressure_cg_gpu.py (N = 17, 32, 40, 64 and five edge sizes) cannot see:

(a) sf_poisson_residual on fields whose shell cells are independent random numbers: every neighbour the stencil reads
    "as stored" — the two wave-uniform i-shell loads, the j-shell rows, the k-shell and ghost planes — is then a value
    of its own, where after set_bnd(0, .) a read of the wrong cell returns the same number;
(b) sf_project_cg at every size of shape_cases.CG_SHAPES (N = 64 W, 64 W + 1, a full and a ragged vector in the second
    trip, a second trip of many lanes, every N mod W) and every decomposition of shape_cases.DECOMPOSED;
(c) runs of 83 to 127 iterations to convergence: alpha and beta rounded once per iteration, the stop on the
    reference's iteration;
(d) signed zeros, infinities and the stop tests' edges;
(e) vel_step with CG selected under the SF_* switches that change what runs in front of, or around, project_cg.

Every comparison is exact equality of bits against tests/pressure_cg_ref.py. tests/test_pressure_cg_inputs_ref.py shows
on the CPU which wrong kernels these inputs tell from the right one, size by size."""
import os

import numpy as np
import pytest

import diagnostics_ref as D
import pressure_cg_ref as R
import shape_cases as C
from gpu_support import CG_STEP_SETTINGS, S, assert_same_bits, check_solve, make, random_fields, upload_all

pytestmark = pytest.mark.gpu

TOL = 1e-3
CASES = [(N, t, 1, "copy") for N, t in C.CG_SHAPES] + [(N, t, P, tr) for N, P, tr in C.DECOMPOSED for t in C.DTYPES]
CASE_IDS = [f"N{n}-{C.dname(t)}-P{p}-{tr}" for n, t, p, tr in CASES]
_REFERENCES = {}


def solve_case(fs, N, dtype, seed, tol, max_iters, what):
    """check_solve on cg_velocity(N, dtype, seed). The decomposed cases solve the inputs of the P = 1 cases: the
    reference of an input is computed once and only read afterwards."""
    u, v, w = C.cg_velocity(N, dtype, seed)
    key = (N, C.dname(dtype), seed, tol, max_iters)
    if key not in _REFERENCES:
        _REFERENCES[key] = R.project_cg(u, v, w, tol, max_iters)
    return check_solve(fs, u, v, w, tol, max_iters, what, want=_REFERENCES[key])


# ---- (a) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype,P,transport", CASES, ids=CASE_IDS)
def test_residual_reads_the_shells_as_stored(N, dtype, P, transport):
    """Both orders of the pair, so that neither array is only ever the right-hand side; nothing is written."""
    p, div = C.stored_shell_pair(N, dtype, C.shell_seed(N))
    with make(N, dtype, P=P, transport=transport) as fs:
        for a, b in ((p, div), (div, p)):
            fs.upload("u0", a)
            fs.upload("v0", b)
            got = fs.poisson_residual("u0", "v0")
            want = R.poisson_residual(a, b)
            print(f"N={N} P={P}: got {got!r} want {want!r}")
            assert D.bits(got) == D.bits(want)
            assert_same_bits(fs.download("u0"), a, "p after the residual")
            assert_same_bits(fs.download("v0"), b, "div after the residual")


# ---- (b) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype,P,transport", CASES, ids=CASE_IDS)
def test_solve_at_every_row_shape(N, dtype, P, transport):
    """Stopped by max_iters = cg_iters(N) from N = 5 on. At N = 1 the one cell is its own mean, r = 0 and there is no
    iteration; at N = 2 and 3 (8 and 27 cells, few distinct eigenvalues) CG is exact within the 8 iterations and the
    reference reports CONVERGED: there the reference alone decides."""
    iters = C.cg_iters(N)
    with make(N, dtype, P=P, transport=transport) as fs:
        want = solve_case(fs, N, dtype, C.cg_seed(N), TOL, iters, f"N={N} P={P} {transport}")
    if N >= 5:
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, iters)
    else:
        assert want["status"] == R.CONVERGED and (want["iterations"] == 0 if N == 1 else 1 <= want["iterations"] <= iters)


# ---- (c) -----------------------------------------------------------------------------------------------------------
LONG = [(34, 1, "copy"), (65, 1, "copy"), (70, 1, "copy"), (34, 17, "rccl-self"), (65, 5, "copy"), (70, 2, "rccl-self")]
LONG_SEED = 2


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
@pytest.mark.parametrize("N,P,transport", LONG, ids=[f"N{n}-P{p}-{t}" for n, p, t in LONG])
def test_long_runs_stop_on_the_reference_iteration(N, P, transport, dtype):
    """tol = 1e-3 on the random velocity: 83 / 113 / 127 iterations at N = 34 / 65 / 70 in either precision. The trace of
    the run stays below the size up to which the schedule-hazard check of tests/conftest.py reads it."""
    with make(N, dtype, P=P, transport=transport) as fs:
        want = solve_case(fs, N, dtype, LONG_SEED, TOL, 400, f"long N={N} P={P} {transport}")
    assert want["status"] == R.CONVERGED and want["iterations"] >= 50
    size = os.path.getsize(os.environ["SF_TRACE_SCHEDULE"].split(",")[0])  # (every context writes its geometry line)
    print(f"schedule trace: {size} bytes")
    assert 0 < size < (64 << 20)


# ---- (d) -----------------------------------------------------------------------------------------------------------
EDGE = [(13, 1, "copy"), (70, 1, "copy"), (70, 2, "rccl-self")]
EDGE_IDS = [f"N{n}-P{p}" for n, p, _ in EDGE]


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
@pytest.mark.parametrize("N,P,transport", EDGE, ids=EDGE_IDS)
def test_zero_velocity_with_a_negative_zero(N, P, transport, dtype):
    """A fixed point of the three set_bnd (u's i-shell is -1 * (+0) = -0), one interior cell -0: no iteration, p = +0 on
    every cell, and the velocity comes back in the bits that went in."""
    u, v, w = (np.zeros((N + 2,) * 3, dtype) for _ in range(3))
    u[N // 2, 3, N] = -0.0
    for b, f in ((1, u), (2, v), (3, w)):
        R.set_bnd(b, f)
    with make(N, dtype, P=P, transport=transport) as fs:
        want = check_solve(fs, u, v, w, TOL, 20, f"zero N={N} P={P}")
        assert (want["status"], want["iterations"], D.bits(want["rel_residual"])) == (R.CONVERGED, 0, D.bits(0.0))
        assert_same_bits(fs.download("u0"), np.zeros_like(u), "p")
        for n, f in (("u", u), ("v", v), ("w", w)):
            assert_same_bits(fs.download(n), f, f"{n} unchanged")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
@pytest.mark.parametrize("value", [np.inf, -np.inf], ids=["+inf", "-inf"])
@pytest.mark.parametrize("N,P,transport", EDGE, ids=EDGE_IDS)
def test_an_infinite_cell_is_a_status(N, P, transport, value, dtype):
    u, v, w = C.cg_velocity(N, dtype, 40 + N)
    bad = w.copy()
    bad[N // 2, 3, 5] = value
    ref = R.project_cg(u, v, bad, TOL, 20)
    with make(N, dtype, P=P, transport=transport) as fs:
        for n, a in (("u", u), ("v", v), ("w", bad)):
            fs.upload(n, a)
        info = fs.project_cg("u", "v", "w", "u0", "v0", TOL, 20)
        fs.sync()
        print(f"got {info} want status {ref['status']} iterations {ref['iterations']} rel {ref['rel_residual']!r}")
        assert (info["status"], info["iterations"]) == (ref["status"], ref["iterations"])
        assert D.bits(info["rel_residual"]) == D.bits(ref["rel_residual"])
        for slot, name in (("u", "u"), ("v", "v"), ("w", "w"), ("u0", "p"), ("v0", "div")):
            assert np.array_equal(np.isnan(fs.download(slot)), np.isnan(ref[name])), name
        check_solve(fs, u, v, w, TOL, 6, "the next solve on the context")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
@pytest.mark.parametrize("N,P,transport", EDGE, ids=EDGE_IDS)
def test_edges_of_the_stop_tests(N, P, transport, dtype):
    """max_iters = 1; tol = 1e30 (any rho' passes: one iteration); tol = 1e-200 (tol * tol underflows to 0 in double, so
    only rho' == 0 would pass: the run ends at max_iters = 12)."""
    u, v, w = C.cg_velocity(N, dtype, 60 + N)
    with make(N, dtype, P=P, transport=transport) as fs:
        want = check_solve(fs, u, v, w, TOL, 1, "max_iters = 1")
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, 1)
        want = check_solve(fs, u, v, w, 1e30, 50, "tol = 1e30")
        assert (want["status"], want["iterations"]) == (R.CONVERGED, 1)
        assert 1e-200 * 1e-200 == 0.0
        want = check_solve(fs, u, v, w, 1e-200, 12, "tol = 1e-200")
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, 12)


# ---- (e) -----------------------------------------------------------------------------------------------------------
SETTINGS = CG_STEP_SETTINGS
VEL_N, VEL_TOL, VEL_MAX, VEL_STEPS = 40, 1e-2, 10, 2
VEL_NAMES = ("u", "v", "w")
_DEFAULT_OUTCOMES = {}


def vel_steps_with_cg(K, bound, P):
    """Two vel_step with CG selected at N = 40 fp32: (u, v, w), and per step the counts and residual bits."""
    dtype = np.float32
    f = random_fields(VEL_N, dtype, 41)
    with make(VEL_N, dtype, K=K, P=P) as fs:
        upload_all(fs, f)
        if bound:
            for slot, n in (("user0", "u0"), ("user1", "v0"), ("user2", "w0")):
                fs.upload(slot, f[n])
            fs.bind_sources("user0", "user1", "user2", None)
        fs.set_pressure_solver("cg", VEL_TOL, VEL_MAX)
        infos = []
        for _ in range(VEL_STEPS):
            fs.vel_step()
            i = fs.pressure_info()
            infos.append((i["solver"], i["status"], i["iterations"], D.bits(i["rel_residual"]), i["solves_total"],
                          i["iterations_total"]))
            if not bound:
                for n in ("u0", "v0", "w0"):  # the sources of the next step
                    fs.upload(n, f[n])
        fs.sync()
        return {n: fs.download(n) for n in VEL_NAMES}, infos


@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("bound", [False, True], ids=["unbound", "bound"])
@pytest.mark.parametrize("K", [6, 9])
def test_vel_step_with_cg_under_switches(K, bound, P, env, monkeypatch):
    """The outcome under the default switches (tied to the single operators by
    test_pressure_cg_gpu.py::test_vel_step_with_cg_is_the_composed_step*) is computed once per (K, bound, P); every
    setting must reproduce it in every bit. op_project_cg mirrors u's i-shell itself where the diffusing kernel left it
    unwritten, which depends on SF_ISHELL, on the Jacobi kernel in front and on bound sources."""
    key = (K, bound, P)
    if key not in _DEFAULT_OUTCOMES:
        _DEFAULT_OUTCOMES[key] = vel_steps_with_cg(K, bound, P)
    want_fields, want_infos = _DEFAULT_OUTCOMES[key]
    assert all(i[0] == S().SF_PRESSURE_CG and i[2] >= 1 for i in want_infos)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got_fields, got_infos = vel_steps_with_cg(K, bound, P)
    assert got_infos == want_infos, env
    for n in VEL_NAMES:
        assert_same_bits(got_fields[n], want_fields[n], f"{env} K={K} bound={bound} P={P}: {n}")


def test_graphs_replay_around_an_uncaptured_cg_step(monkeypatch):
    """SF_GRAPH=1: vel_step with CG selected is not captured (its sums are read on the host) while dens_step and the
    Jacobi vel_step of the same context go through graphs. Jacobi step, dens_step, CG step, dens_step, Jacobi step on
    one context equal the same sequence without graphs. (Whether the steps after the CG step replay a cached graph or
    capture anew — the cache is keyed on the slots' pointers — the library does not report; either way must give these
    bits.)"""
    N, dtype = VEL_N, np.float32
    f = random_fields(N, dtype, 43)
    out = []
    for graph in ("0", "1"):
        monkeypatch.setenv("SF_GRAPH", graph)
        with make(N, dtype, K=6) as fs:
            upload_all(fs, f)
            infos = []
            for solver in ("jacobi", None, "cg", None, "jacobi"):
                if solver is None:
                    fs.dens_step()
                    continue
                fs.set_pressure_solver(solver, VEL_TOL, VEL_MAX)
                fs.vel_step()
                i = fs.pressure_info()
                infos.append((i["solver"], i["status"], i["iterations"], D.bits(i["rel_residual"])))
            fs.sync()
            out.append(({n: fs.download(n) for n in S().FIELD_NAMES}, infos))
    assert out[0][1] == out[1][1]
    assert [i[0] for i in out[0][1]] == [S().SF_PRESSURE_JACOBI, S().SF_PRESSURE_CG, S().SF_PRESSURE_JACOBI]
    for n in S().FIELD_NAMES:
        assert_same_bits(out[1][0][n], out[0][0][n], f"{n}: SF_GRAPH=1 against no graphs")
