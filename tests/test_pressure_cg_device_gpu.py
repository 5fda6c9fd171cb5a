"""The conjugate-gradient projection with its scalars on the device (docs/SPEC.md §11 "Where the scalars are computed",
sf_set_pressure_sync): for every check_every the solve must leave the bits of tests/pressure_cg_ref.py — p, u, v, w, div,
iterations, status, rel_residual — which are also the bits of the check_every = 0 path of the same context.

(1) sizes at which each row shape first appears, both precisions, max_iters = 8, check_every in {1, 3, 8 = max_iters},
    and a run to convergence (83 iterations) with check_every 1 and 7;
(2) every decomposition of shape_cases.DECOMPOSED with check_every = 3: the scalar kernel runs once, on slab 0's stream,
    over the records of all slabs, the other slabs wait for it; rccl-self contexts all-gather the records on the device;
(3) every way a solve stops (tests/pressure_cg_device_model.stop_inputs), with check_every 1 and 5: iterations enqueued
    past the stop must change nothing. tests/test_pressure_cg_device_ref.py shows on the CPU which wrong protocol each
    of these inputs catches;
(4) the host waits of either path (sf_pressure_sync_get);
(5) vel_step + dens_step with CG selected: check_every = 4 against check_every = 0.
The schedule-hazard check of tests/conftest.py reads the trace of every context created here."""
import time

import numpy as np
import pytest

import diagnostics_ref as D
import pressure_cg_device_model as M
import pressure_cg_ref as R
import shape_cases as C
from gpu_support import S, assert_same_bits, check_solve, make, random_fields, upload_all

pytestmark = pytest.mark.gpu

TOL, MAX_ITERS = 1e-3, 8
SIZES = ([(N, t) for N in (1, 2, 3, 5, 13, 34, 65, 70) for t in C.DTYPES]
         + [(129, np.float64), (257, np.float32), (200, np.float64), (324, np.float32)])
SIZE_IDS = [f"N{n}-{C.dname(t)}" for n, t in SIZES]
OUT = (("u", "u"), ("v", "v"), ("w", "w"), ("u0", "p"), ("v0", "div"))
_REFERENCES = {}


def reference(N, dtype, seed, tol, max_iters):
    """R.project_cg of cg_velocity(N, dtype, seed): computed once per input, only read afterwards."""
    key = (N, C.dname(dtype), seed, tol, max_iters)
    if key not in _REFERENCES:
        t0 = time.perf_counter()
        _REFERENCES[key] = R.project_cg(*C.cg_velocity(N, dtype, seed), tol, max_iters)
        print(f"reference {key}: {time.perf_counter() - t0:.1f} s")
    return _REFERENCES[key]


def ceil_div(a, b):
    return -(-a // b)


def solve(fs, m, u, v, w, tol, max_iters, want, what, nan_ok=False):
    """One solve with check_every = m against `want` (a dict of pressure_cg_ref.project_cg), the host waits of that path
    included. Returns the downloaded outputs. nan_ok: inputs that put NaN into the fields — status, counts and residual
    in bits, NaN in the same cells, every other cell in bits."""
    fs.set_pressure_sync(m)
    if nan_ok:
        for n, a in (("u", u), ("v", v), ("w", w)):
            fs.upload(n, a)
        info = fs.project_cg("u", "v", "w", "u0", "v0", tol, max_iters)
        fs.sync()
        print(f"{what}: got {info} want status {want['status']} iterations {want['iterations']} rel {want['rel_residual']!r}")
        assert (info["status"], info["iterations"]) == (want["status"], want["iterations"]), what
        assert D.bits(info["rel_residual"]) == D.bits(want["rel_residual"]) or (
            np.isnan(info["rel_residual"]) and np.isnan(want["rel_residual"])), what
    else:
        check_solve(fs, u, v, w, tol, max_iters, what, want=want)
    got = {name: fs.download(slot) for slot, name in OUT}
    if nan_ok:
        for name in got:
            assert_same_bits(got[name], want[name], f"{what}: {name}", nan_ok=True)
    sync = fs.pressure_sync
    print(f"{what}: {sync}")
    assert sync["check_every"] == m
    if m == 0:
        if want["status"] != R.BREAKDOWN and not (want["status"] == R.CONVERGED and want["iterations"] == 0):
            assert sync["host_waits"] == 2 + 2 * want["iterations"], what  # (the run ended on the rho test)
    else:
        assert 1 <= sync["host_waits"] <= ceil_div(want["iterations"], m) + 1, what
        if m >= max_iters:
            assert sync["host_waits"] == 1, what
    return got


def solve_every_m(fs, ms, u, v, w, tol, max_iters, want, what, nan_ok=False):
    """check_every = 0 first, then every m of ms on the same context: each against the reference and against the bits the
    host path left."""
    host = solve(fs, 0, u, v, w, tol, max_iters, want, f"{what} m=0", nan_ok)
    total = fs.pressure_sync["host_waits_total"]
    for m in ms:
        got = solve(fs, m, u, v, w, tol, max_iters, want, f"{what} m={m}", nan_ok)
        for name in got:
            assert_same_bits(got[name], host[name], f"{what} m={m} against m=0: {name}", nan_ok=nan_ok)
        total += fs.pressure_sync["host_waits"]
        assert fs.pressure_sync["host_waits_total"] == total


# ---- (1) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", SIZES, ids=SIZE_IDS)
def test_bits_at_every_row_shape(N, dtype):
    """The random velocity of the shapes suite, max_iters = 8 = the largest check_every. N = 1: no iteration; N = 2, 3:
    exact within the 8 (the reference decides); from N = 5 on all 8 iterations run."""
    seed = C.cg_seed(N)
    want = reference(N, dtype, seed, TOL, MAX_ITERS)
    if N >= 5:
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, MAX_ITERS)
    u, v, w = C.cg_velocity(N, dtype, seed)
    with make(N, dtype) as fs:
        solve_every_m(fs, (1, 3, MAX_ITERS), u, v, w, TOL, MAX_ITERS, want, f"N={N} {C.dname(dtype)}")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
def test_a_run_to_convergence(dtype):
    """N = 34, seed 2, tol = 1e-3: CONVERGED after 83 iterations. check_every = 7 enqueues one no-op iteration after the
    stop (84 = 12 * 7) and reads the state 12 times; check_every = 1 reads it 83 times."""
    N, seed, limit = 34, 2, 400
    want = reference(N, dtype, seed, TOL, limit)
    assert (want["status"], want["iterations"]) == (R.CONVERGED, 83)
    u, v, w = C.cg_velocity(N, dtype, seed)
    with make(N, dtype) as fs:
        solve_every_m(fs, (1, 7), u, v, w, TOL, limit, want, f"long N={N} {C.dname(dtype)}")
        assert fs.pressure_sync["host_waits"] == 12


# ---- (2) -----------------------------------------------------------------------------------------------------------
DECOMPOSED = [(N, t, P, tr) for N, P, tr in C.DECOMPOSED for t in C.DTYPES]


@pytest.mark.parametrize("N,dtype,P,transport", DECOMPOSED, ids=[f"N{n}-{C.dname(t)}-P{p}-{tr}" for n, t, p, tr in DECOMPOSED])
def test_every_decomposition(N, dtype, P, transport):
    """The inputs and limits of the shapes suite (cg_iters(N) iterations), check_every = 3."""
    seed, iters = C.cg_seed(N), C.cg_iters(N)
    want = reference(N, dtype, seed, TOL, iters)
    u, v, w = C.cg_velocity(N, dtype, seed)
    with make(N, dtype, P=P, transport=transport) as fs:
        solve_every_m(fs, (3,), u, v, w, TOL, iters, want, f"N={N} P={P} {transport}")
        if transport == "rccl-self":  # the records went through the collective, on either path
            assert fs.transport_info()["rccl_groups"] > 0


# ---- (3) -----------------------------------------------------------------------------------------------------------
STOP = M.stop_inputs()
_STOP_REFERENCES = {}


def stop_reference(name):
    if name not in _STOP_REFERENCES:
        u, v, w, tol, max_iters = STOP[name]
        _STOP_REFERENCES[name] = R.project_cg(u, v, w, tol, max_iters)
    return _STOP_REFERENCES[name]


@pytest.mark.parametrize("m", [1, 5], ids=["m1", "m5"])
@pytest.mark.parametrize("name", list(STOP))
def test_stop_cases(name, m):
    """zero: 0 iterations, CONVERGED, the velocity back in the bits that went in; nan, +-inf: BREAKDOWN at iteration 0 or 1;
    max_iters 0 and 1; tol = 1e30 (one iteration) and 1e-200 (never); stop_at_2: CONVERGED at iteration 2 of 8, so that
    check_every = 5 enqueues three iterations that must leave p and `iterations` alone; delta: d.Ad <= 0 after 6 to 22
    iterations, where cg_update must not run any more."""
    u, v, w, tol, max_iters = STOP[name]
    want = stop_reference(name)
    nan_ok = name[:4] in ("nan-", "+inf", "-inf")
    with make(u.shape[0] - 2, u.dtype.type) as fs:
        solve_every_m(fs, (m,), u, v, w, tol, max_iters, want, f"{name} m={m}", nan_ok)
        if name.startswith("zero"):
            assert (want["status"], want["iterations"]) == (R.CONVERGED, 0)
            for n, f in (("u", u), ("v", v), ("w", w)):
                assert_same_bits(fs.download(n), f, f"{n} unchanged")
        if name.startswith("stop_at_2"):
            assert (want["status"], want["iterations"]) == (R.CONVERGED, 2)
            assert fs.pressure_sync["host_waits"] == (2 if m == 1 else 1)
        if nan_ok:  # the context is good for the next solve
            vel = C.cg_velocity(u.shape[0] - 2, u.dtype.type, 5)
            check_solve(fs, *vel, TOL, 6, "the next solve on the context")


@pytest.mark.parametrize("name", ["stop_at_2-f32", "zero-f64", "tol1e-200-f32", "max_iters0-f64"])
def test_stop_cases_on_four_slabs(name):
    u, v, w, tol, max_iters = STOP[name]
    with make(M.STOP_N, u.dtype.type, P=4, transport="rccl-self" if name.endswith("f32") else "copy") as fs:
        solve_every_m(fs, (1, 5), u, v, w, tol, max_iters, stop_reference(name), f"{name} P=4")


# ---- (4) -----------------------------------------------------------------------------------------------------------
def test_host_waits_and_the_setting():
    """The counts of either path on one context, the default, and the argument check."""
    N, dtype = M.STOP_N, np.float32
    u, v, w, tol, max_iters = STOP["stop_at_2-f32"]
    want = stop_reference("stop_at_2-f32")
    with make(N, dtype) as fs:
        assert fs.pressure_sync == {"check_every": 0, "host_waits": 0, "host_waits_total": 0}
        solve(fs, 0, u, v, w, tol, max_iters, want, "host path")
        assert fs.pressure_sync["host_waits"] == 2 + 2 * 2
        solve(fs, 1, u, v, w, tol, max_iters, want, "m=1")
        assert fs.pressure_sync["host_waits"] == 2
        solve(fs, 2, u, v, w, tol, max_iters, want, "m=2")
        assert fs.pressure_sync["host_waits"] == 1
        solve(fs, 8, u, v, w, tol, max_iters, want, "m=max_iters")
        assert fs.pressure_sync["host_waits"] == 1
        solve(fs, 1000, u, v, w, tol, max_iters, want, "m>max_iters")
        assert fs.pressure_sync == {"check_every": 1000, "host_waits": 1, "host_waits_total": 6 + 2 + 1 + 1 + 1}
        with pytest.raises(S().SfError) as e:
            fs.set_pressure_sync(-1)
        assert e.value.status == S().SF_ERR_INVALID
        assert fs.pressure_sync["check_every"] == 1000


# ---- (5) -----------------------------------------------------------------------------------------------------------
def steps_with_cg(P, m):
    """Two vel_step + dens_step with CG selected at N = 40 fp32: the eight fields, and per step the pressure info."""
    N, dtype = 40, np.float32
    f = random_fields(N, dtype, 41)
    with make(N, dtype, K=6, P=P) as fs:
        upload_all(fs, f)
        fs.set_pressure_solver("cg", 1e-2, 10)
        fs.set_pressure_sync(m)
        infos = []
        for _ in range(2):
            fs.vel_step()
            fs.dens_step()
            i = fs.pressure_info()
            infos.append((i["solver"], i["status"], i["iterations"], D.bits(i["rel_residual"]), i["solves_total"],
                          i["iterations_total"]))
            for n in ("u0", "v0", "w0", "dens0"):  # the sources of the next step
                fs.upload(n, f[n])
        fs.sync()
        return {n: fs.download(n) for n in ("u", "v", "w", "dens")}, infos, fs.pressure_sync


@pytest.mark.parametrize("P", [1, 4])
def test_steps_with_cg_selected(P):
    want_fields, want_infos, host_sync = steps_with_cg(P, 0)
    got_fields, got_infos, sync = steps_with_cg(P, 4)
    print(f"P={P}: {got_infos} host path {host_sync} check_every=4 {sync}")
    assert all(i[0] == S().SF_PRESSURE_CG and i[2] >= 1 for i in want_infos)
    assert got_infos == want_infos
    for n in want_fields:
        assert_same_bits(got_fields[n], want_fields[n], f"P={P}: {n}")
    assert sync["check_every"] == 4 and 4 <= sync["host_waits_total"] < host_sync["host_waits_total"]
