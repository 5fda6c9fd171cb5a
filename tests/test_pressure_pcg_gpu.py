"""The Jacobi-sweep preconditioner of the conjugate-gradient projection (docs/SPEC.md §11.2,
sf_set_pressure_preconditioner): every solve must leave the bits of tests/pressure_pcg_ref.py — p, u, v, w, div,
iterations, status, rel_residual and the double of sf_poisson_residual.

(1) the row shapes of the new dot kernel: project_cg with m = 4 at every size class, the second-trip sizes included;
(2) m in {1, 2, 3, 4, 5, 8} at N = 34 and 65 with the default kernels and with the marching kernel forced: a single sweep
    on a really zeroed z everywhere, and at N = 34 in fp64 (the one case here that fuses) the zero-iterate pair, pairs,
    and the zero-iterate and plain marching passes feed a solve;
(3) every decomposition of shape_cases.DECOMPOSED with m = 4 and m = 3 (34 / 17: a ghost plane next to every plane, the
    exchange of r), scalars on the host and on the device;
(4) check_every in {0, 1, 3, 8}: the same bits however the solve stops;
(5) none selected again: today's project_cg, and sf_lin_solve_launches unchanged;
(6) vel_step with CG and jacobi:4 against the step composed in numpy.
tests/test_pressure_pcg_ref.py shows on the CPU which wrong library these inputs tell from the right one. The
schedule-hazard check of tests/conftest.py reads the trace of every context created here."""
import time

import numpy as np
import pytest

import diagnostics_ref as D
import pcg_cases as PC
import pressure_cg_ref as R
import pressure_pcg_ref as Q
import shape_cases as C
from gpu_support import S, assert_same_bits, check_solve, make, march_mode, random_fields, reference_vel_step, upload_all  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = PC.TOL
OUT = (("u", "u"), ("v", "v"), ("w", "w"), ("u0", "p"), ("v0", "div"))
_REFERENCES = {}


def reference(N, dtype, seed, tol, max_iters, m):
    """Q.project_cg of cg_velocity(N, dtype, seed): computed once per input, only read afterwards."""
    key = (N, C.dname(dtype), seed, tol, max_iters, m)
    if key not in _REFERENCES:
        t0 = time.perf_counter()
        _REFERENCES[key] = Q.project_cg(*C.cg_velocity(N, dtype, seed), tol, max_iters, m)
        print(f"reference {key}: {time.perf_counter() - t0:.1f} s")
    return _REFERENCES[key]


def precondition(fs, m):
    if m > 0:
        fs.set_pressure_preconditioner("jacobi", m)
    else:
        fs.set_pressure_preconditioner("none")
    want = {"kind": S().SF_PRECOND_JACOBI if m > 0 else S().SF_PRECOND_NONE, "sweeps": m}
    assert fs.pressure_preconditioner == want


def solve_nan_ok(fs, u, v, w, tol, max_iters, what, want):
    """check_solve for inputs that put NaN into the fields: status, counts and residual as the reference has them, NaN in
    the same cells, every other cell in bits."""
    for n, a in (("u", u), ("v", v), ("w", w)):
        fs.upload(n, a)
    info = fs.project_cg("u", "v", "w", "u0", "v0", tol, max_iters)
    fs.sync()
    print(f"{what}: got {info} want status {want['status']} iterations {want['iterations']} rel {want['rel_residual']!r}")
    assert (info["status"], info["iterations"]) == (want["status"], want["iterations"]), what
    assert D.bits(info["rel_residual"]) == D.bits(want["rel_residual"]) or (
        np.isnan(info["rel_residual"]) and np.isnan(want["rel_residual"])), what
    for slot, name in OUT:
        assert_same_bits(fs.download(slot), want[name], f"{what}: {name}", nan_ok=True)


# ---- (1) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", PC.ROW_SHAPES, ids=[f"N{n}-{C.dname(t)}" for n, t in PC.ROW_SHAPES])
def test_row_shapes_of_the_dot_kernel(N, dtype):
    """m = 4 on the random velocity: to convergence below N = 128, six iterations from there up. N = 1: r = 0 and no
    iteration; the reference decides everywhere."""
    seed, iters = PC.seed(N), PC.max_iters(N)
    want = reference(N, dtype, seed, TOL, iters, PC.M)
    if N >= 128:
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, iters)
    else:
        assert want["status"] == R.CONVERGED and (want["iterations"] == 0) == (N == 1)
    with make(N, dtype) as fs:
        precondition(fs, PC.M)
        check_solve(fs, *C.cg_velocity(N, dtype, seed), TOL, iters, f"N={N} {C.dname(dtype)} m={PC.M}", want=want)


# ---- (2) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
@pytest.mark.parametrize("m", PC.SWEEPS, ids=[f"m{m}" for m in PC.SWEEPS])
@pytest.mark.parametrize("N", PC.SWEEP_SIZES, ids=[f"N{n}" for n in PC.SWEEP_SIZES])
def test_sweep_counts_and_kernel_forms(N, m, dtype, march_mode):
    """To convergence. m = 1 and the last sweep of m = 3 read a z that op_precondition (m = 1) or the pass before has
    really stored. Only N = 34 in fp64 fuses sweeps (N a multiple of W = 2): pairs by default, and with the marching
    kernel forced m = 5 is a pair and a three-sweep pass, m = 8 the zero-iterate marching pass and a plain one. N = 65
    (odd) in both precisions and N = 34 in fp32 (no multiple of W = 4) run single sweeps on a stored zero for every m
    and either kernel setting. The pass plans at sizes that fuse in both precisions, the fp32 marching tile among them,
    are held by tests/test_pressure_pcg_plans_gpu.py. On the host path and with check_every = 3 on the same context."""
    seed = PC.seed(N)
    want = reference(N, dtype, seed, TOL, PC.TO_CONVERGENCE, m)
    assert want["status"] == R.CONVERGED and want["iterations"] >= 8
    u, v, w = C.cg_velocity(N, dtype, seed)
    with make(N, dtype) as fs:
        precondition(fs, m)
        for every in (0, 3):
            fs.set_pressure_sync(every)
            check_solve(fs, u, v, w, TOL, PC.TO_CONVERGENCE, f"N={N} {C.dname(dtype)} m={m} {march_mode} sync={every}", want=want)


# ---- (3) -----------------------------------------------------------------------------------------------------------
DECOMPOSED = [(N, t, P, tr, m) for N, P, tr in C.DECOMPOSED for t in C.DTYPES for m in (4, 3)]


@pytest.mark.parametrize("N,dtype,P,transport,m", DECOMPOSED,
                         ids=[f"N{n}-{C.dname(t)}-P{p}-{tr}-m{m}" for n, t, p, tr, m in DECOMPOSED])
def test_every_decomposition(N, dtype, P, transport, m):
    """Six iterations of the P = 1 input. The sweeps of M(r) run through the two-stream schedule of the Jacobi solves,
    r's ghost planes travel before them, gamma's plane records cross the slabs."""
    seed = PC.seed(N)
    want = reference(N, dtype, seed, TOL, PC.DECOMPOSED_ITERS, m)
    u, v, w = C.cg_velocity(N, dtype, seed)
    with make(N, dtype, P=P, transport=transport) as fs:
        precondition(fs, m)
        for every in (0, 4):
            fs.set_pressure_sync(every)
            check_solve(fs, u, v, w, TOL, PC.DECOMPOSED_ITERS, f"N={N} P={P} {transport} m={m} sync={every}", want=want)
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


# ---- (4) -----------------------------------------------------------------------------------------------------------
STOP_N = 20


def stop_inputs():
    """name -> (u, v, w, tol, max_iters, m): convergence in the middle of a batch, max_iters no multiple of any
    check_every, a zero right-hand side, a NaN in the velocity."""
    out = {}
    for dtype in C.DTYPES:
        t = C.dname(dtype)
        u, v, w = C.cg_velocity(STOP_N, dtype, 7)
        out[f"converges-{t}"] = (u, v, w, 1.5e-3, 100, 4)  # 17 iterations
        out[f"max_iters7-{t}"] = (u, v, w, 1e-3, 7, 2)
        z = np.zeros_like(u)
        out[f"zero-{t}"] = (z, z.copy(), z.copy(), 1e-3, 10, 4)
        bad = v.copy()
        bad[5, 6, 7] = np.nan
        out[f"nan-{t}"] = (u, bad, w, 1e-3, 10, 3)
    return out


STOP = stop_inputs()


@pytest.mark.parametrize("P", [1, 4], ids=["P1", "P4"])
@pytest.mark.parametrize("name", list(STOP))
def test_check_every_leaves_the_same_bits(name, P):
    """check_every in {0, 1, 3, 8} on one context, each against the reference (hence against each other). The converging
    run stops at an iteration that is no multiple of 3 or 8 (asserted), so the batches of 3 and 8 enqueue iterations
    past the stop, whose sweeps run and whose row kernels must not; max_iters = 7 ends inside a batch of 3 and of 8.

    No case stops on gamma: M is a polynomial in A that is positive on A's range, so finite data give r.z > 0; a NaN
    or an infinity in the velocity reaches rho0 first (BREAKDOWN before M is applied), and no input was found on the CPU
    whose sweeps overflow with rho0 finite and gamma not > 0 — cells that overflow do so with the sign of r there, so
    gamma = +inf passes and the next delta, a NaN, ends the solve. The gamma stages are therefore only held to the
    reference on the cases above."""
    u, v, w, tol, max_iters, m = STOP[name]
    dtype = u.dtype.type
    want = Q.project_cg(u, v, w, tol, max_iters, m)
    if name.startswith("converges"):
        assert want["status"] == R.CONVERGED and want["iterations"] % 3 and want["iterations"] % 8
    if name.startswith("max_iters7"):
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, 7)
    if name.startswith("zero"):
        assert (want["status"], want["iterations"]) == (R.CONVERGED, 0)
    if name.startswith("nan"):
        assert (want["status"], want["iterations"]) == (R.BREAKDOWN, 0)
    with make(STOP_N, dtype, P=P, transport="rccl-self" if dtype == np.float32 else "copy") as fs:
        precondition(fs, m)
        for every in (0, 1, 3, 8):
            fs.set_pressure_sync(every)
            what = f"{name} P={P} check_every={every}"
            if name.startswith("nan"):
                solve_nan_ok(fs, u, v, w, tol, max_iters, what, want)
            else:
                check_solve(fs, u, v, w, tol, max_iters, what, want=want)
            if every >= max_iters:
                assert fs.pressure_sync["host_waits"] == 1
        if name.startswith("nan"):  # the context is good for the next solve
            vel = C.cg_velocity(STOP_N, dtype, 5)
            check_solve(fs, *vel, TOL, 6, "the next solve on the context", want=Q.project_cg(*vel, TOL, 6, m))


# ---- (5) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2], ids=["P1", "P2"])
def test_none_selected_again_is_the_unpreconditioned_solve(P):
    """Default none; jacobi:4 set, used and unset: the bits of pressure_cg_ref, the host waits of §11 and the launch count
    of a Jacobi solve as before. Invalid settings are refused and change nothing."""
    N, dtype = 34, np.float64
    u, v, w = C.cg_velocity(N, dtype, C.cg_seed(N))
    with make(N, dtype, P=P) as fs:
        assert fs.pressure_preconditioner == {"kind": S().SF_PRECOND_NONE, "sweeps": 0}
        launches = [fs.lin_solve_launches(k) for k in range(0, 25)]
        plain = check_solve(fs, u, v, w, TOL, 8, "none (the default)")
        waits = fs.pressure_sync["host_waits"]
        precondition(fs, 4)
        want = reference(N, dtype, C.cg_seed(N), TOL, 8, 4)
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, 8)
        check_solve(fs, u, v, w, TOL, 8, "jacobi:4", want=want)
        assert fs.pressure_sync["host_waits"] == 3 + 3 * 8  # (mu, rho0, gamma0; delta, rho', gamma' per iteration)
        fs.set_pressure_preconditioner("none", 4)
        assert fs.pressure_preconditioner == {"kind": S().SF_PRECOND_NONE, "sweeps": 4}  # kept, not used
        check_solve(fs, u, v, w, TOL, 8, "none again", want=plain)
        assert fs.pressure_sync["host_waits"] == waits == 2 + 2 * 8
        assert [fs.lin_solve_launches(k) for k in range(0, 25)] == launches
        for kind, sweeps in ((S().SF_PRECOND_JACOBI, 0), (S().SF_PRECOND_JACOBI, -1), (2, 4), (-1, 1),
                             (S().SF_PRECOND_NONE, -1)):
            with pytest.raises(S().SfError) as e:
                fs.set_pressure_preconditioner(kind, sweeps)
            assert e.value.status == S().SF_ERR_INVALID
        assert fs.pressure_preconditioner == {"kind": S().SF_PRECOND_NONE, "sweeps": 4}
        for every in (0, 3):
            fs.set_pressure_sync(every)
            check_solve(fs, u, v, w, TOL, 8, f"none, check_every={every}", want=plain)


# ---- (6) -----------------------------------------------------------------------------------------------------------
_STEP_REFERENCE = {}


@pytest.mark.parametrize("every", [0, 4], ids=["host", "sync4"])
@pytest.mark.parametrize("P", [1, 4], ids=["P1", "P4"])
def test_vel_step_with_the_preconditioner(P, every):
    """Two vel_step at N = 40 fp32 with CG (1e-2, 10) and jacobi:4, the sources uploaded again in between."""
    N, dtype, K, tol, max_iters, m = 40, np.float32, 6, 1e-2, 10, 4
    f = random_fields(N, dtype, 41)
    if "want" not in _STEP_REFERENCE:
        g, outs = dict(f), []
        for _ in range(2):
            out = reference_vel_step(g, K, tol, max_iters, m)
            outs.append(out)
            g = dict(f, u=out["u"], v=out["v"], w=out["w"])
        _STEP_REFERENCE["want"] = outs
    outs = _STEP_REFERENCE["want"]
    assert all(o["iterations"] >= 1 for o in outs)
    with make(N, dtype, K=K, P=P) as fs:
        upload_all(fs, f)
        fs.set_pressure_solver("cg", tol, max_iters)
        fs.set_pressure_sync(every)
        precondition(fs, m)
        for step, out in enumerate(outs):
            fs.vel_step()
            info = fs.pressure_info()
            print(f"P={P} step {step}: {info}")
            assert (info["solver"], info["status"], info["iterations"]) == (S().SF_PRESSURE_CG, out["status"], out["iterations"])
            assert D.bits(info["rel_residual"]) == D.bits(out["rel_residual"])
            for n in ("u", "v", "w"):
                assert_same_bits(fs.download(n), out[n], f"P={P} step {step}: {n}")
            for n in ("u0", "v0", "w0"):  # the sources of the next step
                fs.upload(n, f[n])
