"""The numpy reference of the preconditioned CG projection (tests/pressure_pcg_ref.py, docs/SPEC.md §11.2) against closed
forms and itself, the iteration counts that motivate the operator, and — in the style of
tests/test_pressure_cg_inputs_ref.py — the plausible errors of the library written into a *copy* of the reference in
this file, each shown to change a compared bit on an input that tests/test_pressure_pcg_gpu.py runs (or, where no input
can show it, shown to be the reference, and said so). No GPU needed.

Mutants (pcg_copy):
  alpha_rho      alpha = rho / delta, the numerator of §11, instead of gamma / delta
  z_not_zeroed   the sweeps of M(r) start from the z of the solve before (zeros only the first time) instead of +0
  no_last_set_bnd  the last set_bnd(0, z) of the sweeps left out
  d_from_r       d = r + beta d, the direction of §11
  gamma_one_trip gamma summed with second-trip cells added to lane 0 one after another
  stale_r        slab emulation: every slab runs each fused pass of M(r) with the r of the update before on the planes
                 beyond its own (r's ghost planes not exchanged; zeros the first time)
"""
import math

import numpy as np
import pytest

import diagnostics_ref as D
import pcg_cases as PC
import pressure_cg_ref as R
import pressure_pcg_ref as Q
import shape_cases as C
import stable_ref as S3
from gpu_support import DTYPE_IDS, DTYPES
from ref_support import LD, modes, product, row_partials_one_trip, same_bits

I = R.I
F64 = np.float64
SWEEPS = PC.SWEEPS
FIELDS = ("u", "v", "w", "p", "div")


def same_outcome(a, b):
    """Everything the GPU tests compare."""
    return ((a["status"], a["iterations"]) == (b["status"], b["iterations"])
            and D.bits(a["rel_residual"]) == D.bits(b["rel_residual"])
            and all(same_bits(a[n], b[n]) for n in FIELDS)
            and D.bits(R.poisson_residual(a["p"], a["div"])) == D.bits(R.poisson_residual(b["p"], b["div"])))


def mode_velocity(N, m, amps, dtype):
    """u = U psi phi phi, v = V phi psi phi, w = W phi phi psi of SPEC §7.1."""
    (cx, sx), (cy, sy), (cz, sz) = (modes(N, q) for q in m)
    U, V, W = amps
    f = (LD(U) * product(cz, cy, sx), LD(V) * product(cz, sy, cx), LD(W) * product(sz, cy, cx))
    return [np.ascontiguousarray(a.astype(dtype)) for a in f]


# ---- closed forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("m", SWEEPS)
@pytest.mark.parametrize("N,mode", [(8, (1, 1, 1)), (16, (2, 5, 3))])
def test_a_single_mode_is_solved_in_one_iteration_for_every_m(N, mode, m, dtype):
    """div = D M is an eigenvector of A, and M(r) is a polynomial in A: z is a multiple of r and the first direction
    is the answer, whatever m."""
    u, v, w = mode_velocity(N, mode, (0.6, -0.4, 0.9), dtype)
    out = Q.project_cg(u, v, w, 1e-3, 50, m)
    assert (out["status"], out["iterations"]) == (Q.CONVERGED, 1), (out["status"], out["iterations"], out["rel_residual"])
    plain = R.project_cg(u, v, w, 1e-3, 50)
    scale = float(np.max(np.abs(plain["p"])))
    assert float(np.max(np.abs(out["p"].astype(F64) - plain["p"].astype(F64)))) <= 64 * float(np.finfo(dtype).eps) * scale
    assert R.poisson_residual(out["p"], out["div"]) <= 64 * float(np.finfo(dtype).eps)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_zero_velocity_is_left_alone(dtype):
    N = 9
    z = np.zeros((N + 2,) * 3, dtype)
    z[3, 4, 5] = -0.0
    out = Q.project_cg(z, z, z, 1e-3, 10, 4)
    assert (out["status"], out["iterations"], out["rel_residual"]) == (Q.CONVERGED, 0, 0.0)
    assert not out["p"].any() and not np.signbit(out["p"]).any()
    for n in "uvw":
        assert same_bits(out[n][I, I, I], z[I, I, I])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_nan_in_the_velocity_is_a_breakdown(dtype):
    u, v, w = R.smooth_velocity(12, dtype)
    u[5, 6, 7] = np.nan
    out = Q.project_cg(u, v, w, 1e-3, 20, 4)
    assert (out["status"], out["iterations"]) == (Q.BREAKDOWN, 0) and np.isnan(out["rel_residual"])


def test_no_sweeps_is_the_unpreconditioned_reference():
    u, v, w = C.cg_velocity(13, np.float32, C.cg_seed(13))
    assert same_outcome(Q.project_cg(u, v, w, 1e-3, 8, 0), R.project_cg(u, v, w, 1e-3, 8))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", [8, 20])
def test_emulated_slabs_give_the_same_bits(N, dtype):
    u, v, w = C.cg_velocity(N, dtype, N)
    one = Q.project_cg(u, v, w, 1e-2, 6, 4)
    for slabs in (2, 4):
        assert same_outcome(Q.project_cg(u, v, w, 1e-2, 6, 4, slabs=slabs), one)


def test_preconditioner_is_the_projects_sweeps_from_zero():
    """z = M(r) is what §3 project's lin_solve leaves in p: the oracle's project on a velocity whose div is r."""
    rng = np.random.RandomState(5)
    N = 10
    r = rng.standard_normal((N,) * 3).astype(np.float32)
    rhs = np.zeros((N + 2,) * 3, np.float32)
    rhs[I, I, I] = r
    for m in (1, 4):
        p = np.zeros_like(rhs)
        p[2, 3, 4] = 7.0  # (the reference zeroes its iterate itself: this is not read)
        want = np.zeros_like(rhs)
        S3.lin_solve(0, want, rhs, 1, 6, m)
        assert same_bits(Q.precondition(r, m), want)


# ---- iteration counts (SPEC §11.1's table) ----------------------------------------------------------------------------
# measured with this reference (the real §10 tree) on §11.1's smooth field in fp32 at tol = 1e-3: iterations for m = 0,
# 1, 2, 3, 4, 8
MEASURED = {32: {0: 11, 1: 11, 2: 6, 3: 6, 4: 5, 8: 4}, 64: {0: 22, 2: 12, 4: 9, 8: 6}}


@pytest.mark.parametrize("N", [32, 64])
def test_four_sweeps_halve_the_iterations(N):
    """iterations(m = 4) <= 1/2 iterations(m = 0) on the smooth field (plain sums gave about 0.36; the half leaves room
    for the tree sums), every run CONVERGED with a true residual within 4 tol, and m = 1 — a pure scaling of r by 1/6 —
    takes the unpreconditioned count."""
    u, v, w = R.smooth_velocity(N, np.float32)
    got = {}
    for m in MEASURED[N]:
        out = Q.project_cg(u, v, w, 1e-3, 100, m)
        res = R.poisson_residual(out["p"], out["div"])
        print(f"N={N} m={m}: iterations {out['iterations']} recurrence {out['rel_residual']:.4e} true {res:.4e}")
        assert out["status"] == Q.CONVERGED and out["rel_residual"] <= 1e-3 and res <= 4e-3
        got[m] = out["iterations"]
    assert 2 * got[4] <= got[0]
    if 1 in got:
        assert got[1] == got[0]
    assert got == MEASURED[N]


# ---- the copy of the reference, with the mutants ----------------------------------------------------------------------
def tree_sum_one_trip(terms, dtype):
    rows = row_partials_one_trip(terms, D.vec_width(dtype))
    a = np.zeros((rows.shape[0], D.pad_pow2(rows.shape[1])), F64)
    a[:, :rows.shape[1]] = rows
    with np.errstate(all="ignore"):
        return D.total(D.halve(a))


def passes_of(m):
    """The fused passes of an m-sweep solve where pairs are fused and the marching kernel is not taken: 2, 2, ..., (1)."""
    return [2] * (m // 2) + [1] * (m % 2)


def sweeps(z, rhs, n, last_set_bnd=True):
    """n sweeps of §3 lin_solve(0, z, rhs, 1, 6, .) on a copy of z."""
    T = z.dtype.type
    cur = z
    for it in range(n):
        nxt = np.zeros_like(cur)
        nxt[I, I, I] = S3.SPEC.sweep(cur, rhs, T(1), T(1) / T(6), it)
        if last_set_bnd or it < n - 1:
            S3.set_bnd(0, nxt)
        cur = nxt
    return cur


def pcg_copy(u, v, w, tol, max_iters, m, mut=None, slabs=1):
    """pressure_pcg_ref.project_cg (m >= 1) with mutation `mut` (None: the reference, line by line)."""
    dtype = u.dtype
    T = dtype.type
    N = u.shape[0] - 2
    state = {"z": np.zeros((N + 2,) * 3, dtype), "r_old": np.zeros((N,) * 3, dtype)}

    def precondition(r):
        rhs = np.zeros((N + 2,) * 3, dtype)
        rhs[I, I, I] = r
        z0 = state["z"] if mut == "z_not_zeroed" else np.zeros_like(rhs)
        if mut == "stale_r":
            nzl = N // slabs
            stale = np.zeros_like(rhs)
            stale[I, I, I] = state["r_old"]
            z = z0
            for s in passes_of(m):
                nxt = np.zeros_like(z)
                for g in range(slabs):
                    a, b = 1 + g * nzl, 1 + (g + 1) * nzl  # the slab's planes [a, b)
                    seen = stale.copy()
                    seen[a:b] = rhs[a:b]
                    lo, hi = (0 if g == 0 else a), (N + 2 if g == slabs - 1 else b)  # wall slabs own the shell planes
                    nxt[lo:hi] = sweeps(z, seen, s)[lo:hi]
                z = nxt
        else:
            z = sweeps(z0, rhs, m, mut != "no_last_set_bnd")
        state["z"], state["r_old"] = z, r
        return z

    def gamma_of(r, z):
        if mut == "gamma_one_trip":
            with np.errstate(all="ignore"):
                return tree_sum_one_trip(r.astype(F64) * z[I, I, I].astype(F64), dtype)
        return R.dot(r, z[I, I, I], dtype, slabs)

    u, v, w = u.copy(), v.copy(), w.copy()
    with np.errstate(all="ignore"):
        p, div = R.divergence(u, v, w)
        s = R.tree_sum(div[I, I, I].astype(F64), dtype, slabs)
        mu = T(s / float(N) ** 3)
        r = div[I, I, I] - mu
        rho0 = rho = last = R.dot(r, r, dtype, slabs)
        status, iters = Q.MAX_ITERS, 0
        if rho0 == 0.0:
            status = Q.CONVERGED
        elif not math.isfinite(rho0):
            status = Q.BREAKDOWN
        else:
            z = precondition(r)
            gamma = gamma_of(r, z)
            if not gamma > 0.0:
                status = Q.BREAKDOWN
            else:
                d = np.zeros_like(u)
                d[I, I, I] = z[I, I, I]
                R.set_bnd(0, d)
                for n in range(max_iters):
                    q = R.apply_A(d)
                    delta = R.dot(d[I, I, I], q, dtype, slabs)
                    if not delta > 0.0:
                        status = Q.BREAKDOWN
                        break
                    aT = T((rho if mut == "alpha_rho" else gamma) / delta)
                    p[I, I, I] = p[I, I, I] + aT * d[I, I, I]
                    r = r - aT * q
                    rho = last = R.dot(r, r, dtype, slabs)
                    iters = n + 1
                    if not math.isfinite(rho):
                        status = Q.BREAKDOWN
                        break
                    if rho <= (tol * tol) * rho0:
                        status = Q.CONVERGED
                        break
                    z = precondition(r)
                    gamma_new = gamma_of(r, z)
                    if not gamma_new > 0.0:
                        status = Q.BREAKDOWN
                        break
                    bT = T(gamma_new / gamma)
                    d[I, I, I] = (r if mut == "d_from_r" else z[I, I, I]) + bT * d[I, I, I]
                    R.set_bnd(0, d)
                    gamma = gamma_new
        R.set_bnd(0, p)
        R.subtract_gradient(u, v, w, p)
        rel = 0.0 if rho0 == 0.0 else math.sqrt(last / rho0) if last / rho0 >= 0 else float("nan")
    return {"u": u, "v": v, "w": w, "p": p, "div": div, "status": status, "iterations": iters, "rel_residual": rel}


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("m", SWEEPS)
def test_sweep_count_inputs_tell_the_sequence_mutants(m, dtype):
    """The inputs of the GPU file's sweep-count cases: cg_velocity at N = 34 (seed cg_seed(34)), tol = 1e-3, run to
    convergence. alpha_rho and d_from_r are caught for every m and both precisions; z_not_zeroed for every m (the
    kernels can only get it wrong where the first pass is not a fused one — m = 1 — but the input tells it everywhere).

    no_last_set_bnd: no input can show it. Of z only interior cells are ever read — by the sum r.z and by d = z, whose
    shells set_bnd(0, d) writes afresh — so the mutant is the reference on every case (asserted here). It is listed to
    say so: the library may leave z's i-shell unwritten."""
    u, v, w = C.cg_velocity(34, dtype, C.cg_seed(34))
    want = Q.project_cg(u, v, w, 1e-3, 400, m)
    print(f"m={m} {C.dname(dtype)}: status {want['status']} iterations {want['iterations']} rel {want['rel_residual']!r}")
    assert want["status"] == Q.CONVERGED and want["iterations"] >= 8
    assert same_outcome(pcg_copy(u, v, w, 1e-3, 400, m), want), "the copy is not the reference"
    for mut in ("alpha_rho", "d_from_r", "z_not_zeroed"):
        assert not same_outcome(pcg_copy(u, v, w, 1e-3, 400, m, mut), want), mut
    assert same_outcome(pcg_copy(u, v, w, 1e-3, 400, m, "no_last_set_bnd"), want)


def test_second_trip_input_tells_gamma_summed_in_one_trip():
    """cg_velocity at N = 131 in fp64 (a second trip of a full vector and a ragged one), m = 4, max_iters = 6: the row
    shape case of the GPU file, at the seed of pcg_cases (the second trip is two vectors of a row: few sums of a run
    see their order, and at seed 500 + N none of the seven r.z does). At N = 34 (one trip) the mutant is the
    reference."""
    u, v, w = C.cg_velocity(131, np.float64, PC.seed(131))
    want = Q.project_cg(u, v, w, 1e-3, 6, 4)
    assert (want["status"], want["iterations"]) == (Q.MAX_ITERS, 6)
    assert not same_outcome(pcg_copy(u, v, w, 1e-3, 6, 4, "gamma_one_trip"), want)
    u, v, w = C.cg_velocity(34, np.float64, C.cg_seed(34))
    assert same_outcome(pcg_copy(u, v, w, 1e-3, 6, 4, "gamma_one_trip"), Q.project_cg(u, v, w, 1e-3, 6, 4))


STALE = [(34, 17, np.float64, 4), (34, 17, np.float64, 3), (34, 2, np.float64, 4), (40, 4, np.float32, 4)]


@pytest.mark.parametrize("N,P,dtype,m", STALE, ids=[f"N{n}-P{p}-{C.dname(t)}-m{m}" for n, p, t, m in STALE])
def test_decomposed_inputs_tell_stale_ghost_planes_of_r(N, P, dtype, m):
    """The decomposed cases of the GPU file where pairs of sweeps are fused (N a multiple of W: 34 in fp64, 40 in
    fp32): a pass of two sweeps evaluates its first one on the plane next to the slab and reads r there. With r's ghost
    planes left as the update before had them the solve differs from the first iteration on; with one sweep per pass
    (m = 1) nothing beyond the slab's own planes is read and the mutant is the reference."""
    u, v, w = C.cg_velocity(N, dtype, C.cg_seed(N))
    want = Q.project_cg(u, v, w, 1e-3, 6, m, slabs=P)
    assert same_outcome(want, Q.project_cg(u, v, w, 1e-3, 6, m))
    assert not same_outcome(pcg_copy(u, v, w, 1e-3, 6, m, "stale_r", slabs=P), want)
    one = Q.project_cg(u, v, w, 1e-3, 6, 1, slabs=P)
    assert same_outcome(pcg_copy(u, v, w, 1e-3, 6, 1, "stale_r", slabs=P), one)
