"""The inputs of tests/test_pressure_cg_shapes_gpu.py discriminate (no GPU needed): the counterpart of
tests/test_shape_inputs_ref.py for SPEC §11. Each plausible error of the four CG kernels or of the host sequence is
written into a *copy* of tests/pressure_cg_ref.py in this file (never into the reference or the library). The unmutated
copy equals the reference in every compared bit wherever a mutant is run through it (asserted: the residual at every
size, the solve up to N = 200 and on the long runs; above 200 no mutated solve is run), each mutant must change at least one compared
bit — status, iteration count, rel_residual, a field, or the double of poisson_residual — at the sizes where the kernel
form can go wrong that way, and must equal the reference at the sizes that are known to be blind to it, so that the
reason for every size of shape_cases.CG_SHAPES is written down in executable form.

The inputs are those of the GPU file: (a) `stored_shell_pair` under poisson_residual, (b) `cg_velocity` under project_cg
stopped by max_iters = cg_iters(N), (c) the same run to convergence at tol = 1e-3.

Mutants of the stencil (cg_stencil reads the i-shell through two wave-uniform loads, the j-shell as rows, the k-shell or
ghost planes as planes):
  mirror_{i,j,k}_{lo,hi,both}  the mirrored interior cell instead of the stored shell cell
  seam_hi   the last cell of a stretch of 64 W cells takes the shell cell x[N+1] as its right neighbour
  seam_lo   the first cell of the next stretch takes x[0] as its left neighbour
Mutants of the sums:
  one_trip  second-trip cells added to lane 0 one after another (mutation 6 of test_shape_inputs_ref.py)
  ragged    the mask of the ragged last vector off by one: the sum takes the shell cell N+1 too. (Of `r` and `q` only
            interior cells are ever stored, so this one is run on (a), where every operand has a stored shell.)
  t_products  products formed in T, then converted to double
Mutants of the host sequence:
  alpha_double, beta_double  the scalar kept in double where a cell uses it (the C++ expression p[e] + alpha * d[e] with
            a double alpha: operands promoted, the result rounded to T once)
  mu_zero, mu_in_T  no mean removed; the mean divided in T: (T)s / (T)N^3
  no_set_bnd  set_bnd(0, d) left out after the direction update
  sqrt_stop   stop on sqrt(rho'/rho0) <= tol instead of rho' <= tol^2 rho0
"""
import math

import numpy as np
import pytest

import diagnostics_ref as D
import pressure_cg_ref as R
import shape_cases as C
from ref_support import row_partials_one_trip, same_bits

I, P, M = R.I, R.P, R.M
F64 = np.float64
TOL = 1e-3
LONG = [(34, 83), (65, 113), (70, 127)]  # (c): N, iterations of the reference at seed 2 in both precisions
LONG_SEED, LONG_MAX = 2, 400
SHELLS = [f"mirror_{a}_{e}" for a in "ijk" for e in ("lo", "hi", "both")]


def two_trip(N, dtype):
    return C.second_trip(N, dtype)


def ragged(N, dtype):
    return N % D.vec_width(dtype) != 0


def sid(s):
    return f"N{s[0]}-{C.dname(s[1])}"


# ---- mutated stencils ----------------------------------------------------------------------------------------------
def apply_A_mut(x, kind):
    """pressure_cg_ref.apply_A with one of the stencil mutations; kind None is the reference expression."""
    T = x.dtype.type
    N = x.shape[0] - 2
    im, ip, jm, jp, km, kp = x[I, I, M], x[I, I, P], x[I, M, I], x[I, P, I], x[M, I, I], x[P, I, I]
    if kind and kind.startswith("mirror"):
        _, axis, end = kind.split("_")
        lo, hi = end in ("lo", "both"), end in ("hi", "both")
        if axis == "i":
            im, ip = im.copy(), ip.copy()
            if lo:
                im[:, :, 0] = x[I, I, 1]
            if hi:
                ip[:, :, -1] = x[I, I, N]
        if axis == "j":
            jm, jp = jm.copy(), jp.copy()
            if lo:
                jm[:, 0, :] = x[I, 1, I]
            if hi:
                jp[:, -1, :] = x[I, N, I]
        if axis == "k":
            km, kp = km.copy(), kp.copy()
            if lo:
                km[0] = x[1, I, I]
            if hi:
                kp[-1] = x[N, I, I]
    if kind in ("seam_hi", "seam_lo"):
        S = D.LANES * D.vec_width(x.dtype)
        im, ip = im.copy(), ip.copy()
        for s in range(S, N, S):  # cell s ends a stretch, cell s + 1 begins the next (s < N)
            if kind == "seam_hi":
                ip[:, :, s - 1] = x[I, I, N + 1]
            else:
                im[:, :, s] = x[I, I, 0]
    return T(6) * x[I, I, I] - (((im + ip) + (jm + jp)) + (km + kp))


def apply_A_with_shell_column(x):
    """apply_A on the cells i = 1 .. N+1 of the interior rows: what a vector that holds the shell cell N+1 computes
    there. The right neighbour of cell N+1 is the next cell in memory, x[k, j+1, 0]."""
    T = x.dtype.type
    N = x.shape[0] - 2
    c = x[I, I, 1:]
    right = np.concatenate([x[I, I, 2:], x[I, 2:, 0:1]], axis=2)
    return T(6) * c - (((x[I, I, :-1] + right) + (x[I, M, 1:] + x[I, P, 1:])) + (x[M, I, 1:] + x[P, I, 1:]))


# ---- mutated sums --------------------------------------------------------------------------------------------------
def fold_rows(rows, dtype):
    a = np.zeros((rows.shape[0], D.pad_pow2(rows.shape[1])), F64)
    a[:, :rows.shape[1]] = rows
    with np.errstate(all="ignore"):
        return D.total(D.halve(a))


def tree_sum_one_trip(terms, dtype, slabs=1):
    with np.errstate(all="ignore"):
        return fold_rows(row_partials_one_trip(terms, D.vec_width(dtype)), dtype)


def tree_sum_with_shell_column(terms, dtype):
    """terms: (N, N, N+1), the last column the shell cell N+1: it is added where the ragged last vector holds it, after
    cell N in the same lane. With N mod W == 0 no vector holds it."""
    nk, N, _ = terms.shape
    W = D.vec_width(dtype)
    if N % W == 0:
        return R.tree_sum(np.ascontiguousarray(terms[:, :, :N]), dtype)
    nm = -(-N // (D.LANES * W))
    t = np.zeros((nk, N, nm * D.LANES * W), F64)
    t[:, :, :N + 1] = terms
    t = t.reshape(nk, N, nm, D.LANES, W)
    c = np.zeros((nk, N, D.LANES), F64)
    with np.errstate(all="ignore"):
        for m in range(nm):
            for e in range(W):
                c = c + t[:, :, m, :, e]
        return fold_rows(D.halve(c), dtype)


# ---- the copy of the reference -------------------------------------------------------------------------------------
def residual_copy(p, div, mut=None, dd=None):
    """pressure_cg_ref.poisson_residual with mutation `mut`. dd: the sum of div.div, where the caller has it already and
    the mutant is one of the stencil (which that sum does not see)."""
    dtype = p.dtype
    with np.errstate(all="ignore"):
        if mut == "ragged":
            e = div[I, I, 1:] - apply_A_with_shell_column(p)
            dv = div[I, I, 1:].astype(F64)
            ee = tree_sum_with_shell_column(e.astype(F64) * e.astype(F64), dtype)
            dd = tree_sum_with_shell_column(dv * dv, dtype)
        else:
            ts = tree_sum_one_trip if mut == "one_trip" else R.tree_sum
            e = div[I, I, I] - apply_A_mut(p, mut)
            dv = div[I, I, I].astype(F64)
            ee = ts(e.astype(F64) * e.astype(F64), dtype)
            if dd is None or mut == "one_trip":
                dd = ts(dv * dv, dtype)
        if dd == 0.0:
            return 0.0
        x = ee / dd
        return math.sqrt(x) if x >= 0 else float("nan")


def cg_copy(u, v, w, tol, max_iters, mut=None, history=None):
    """pressure_cg_ref.project_cg with mutation `mut` (None: the reference, line by line)."""
    dtype = u.dtype
    T = dtype.type
    N = u.shape[0] - 2
    tree_sum = tree_sum_one_trip if mut == "one_trip" else R.tree_sum
    stencil = mut if mut in SHELLS + ["seam_hi", "seam_lo"] else None

    def dot(a, b):
        with np.errstate(all="ignore"):
            terms = (a * b).astype(F64) if mut == "t_products" else a.astype(F64) * b.astype(F64)
            return tree_sum(terms, dtype)

    def axpy(y, s, x, in_double):
        """y + s*x per cell: s rounded to T once (SPEC), or (mutant) the C++ expression with a double s."""
        if in_double:
            return (y.astype(F64) + s * x.astype(F64)).astype(dtype)
        return y + T(s) * x

    u, v, w = u.copy(), v.copy(), w.copy()
    with np.errstate(all="ignore"):
        p, div = R.divergence(u, v, w)
        s = tree_sum(div[I, I, I].astype(F64), dtype)
        mu = T(s / float(N) ** 3)
        if mut == "mu_zero":
            mu = T(0)
        if mut == "mu_in_T":
            mu = T(s) / T(float(N) ** 3)
        r = div[I, I, I] - mu
        d = np.zeros_like(u)
        d[I, I, I] = r
        R.set_bnd(0, d)
        rho0 = rho = last = dot(r, r)
        status, iters = R.MAX_ITERS, 0
        if rho0 == 0.0:
            status = R.CONVERGED
        elif not math.isfinite(rho0):
            status = R.BREAKDOWN
        else:
            for n in range(max_iters):
                q = apply_A_mut(d, stencil)
                delta = dot(d[I, I, I], q)
                if not delta > 0.0:
                    status = R.BREAKDOWN
                    break
                alpha = rho / delta
                p[I, I, I] = axpy(p[I, I, I], alpha, d[I, I, I], mut == "alpha_double")
                r = axpy(r, -alpha, q, mut == "alpha_double")
                rho_new = last = dot(r, r)
                iters = n + 1
                if history is not None:
                    history.append(rho_new)
                if not math.isfinite(rho_new):
                    status = R.BREAKDOWN
                    break
                if (math.sqrt(rho_new / rho0) <= tol) if mut == "sqrt_stop" else (rho_new <= (tol * tol) * rho0):
                    status = R.CONVERGED
                    break
                d[I, I, I] = axpy(r, rho_new / rho, d[I, I, I], mut == "beta_double")
                if mut != "no_set_bnd":
                    R.set_bnd(0, d)
                rho = rho_new
        R.set_bnd(0, p)
        R.subtract_gradient(u, v, w, p)
        rel = 0.0 if rho0 == 0.0 else math.sqrt(last / rho0) if last / rho0 >= 0 else float("nan")
    return {"u": u, "v": v, "w": w, "p": p, "div": div, "status": status, "iterations": iters, "rel_residual": rel}


def same_outcome(a, b):
    """Everything check_solve of the GPU tests compares."""
    return ((a["status"], a["iterations"]) == (b["status"], b["iterations"])
            and D.bits(a["rel_residual"]) == D.bits(b["rel_residual"])
            and all(same_bits(a[n], b[n]) for n in ("u", "v", "w", "p", "div"))
            and D.bits(R.poisson_residual(a["p"], a["div"])) == D.bits(R.poisson_residual(b["p"], b["div"])))


# ---- (a) the as-stored residual ------------------------------------------------------------------------------------
RESIDUAL_SHAPES = C.CG_SHAPES + [(260, np.float32)]  # (260 fp32: the known-blind two-trip size of the older GPU file)
ONE_TRIP_CAUGHT = {(200, np.float64), (131, np.float64), (324, np.float32), (262, np.float32)}
ONE_TRIP_BLIND = {(130, np.float64), (129, np.float64), (260, np.float32), (257, np.float32)}


@pytest.mark.parametrize("N,dtype", RESIDUAL_SHAPES, ids=[sid(s) for s in RESIDUAL_SHAPES])
def test_stored_shells_tell_the_residual_mutants(N, dtype):
    """poisson_residual on stored_shell_pair: every shell mutant is caught at every N; a seam mutant at every two-trip
    size and at no other; the one-trip sum at 200 / 131 (fp64), 324 / 262 (fp32) and not at 130 / 129, 260 / 257 (the
    second trip there is lane 0's one vector, full or ragged, which lane 0 adds after its first in either order); the
    ragged mask at every N mod W != 0 and at no other. (The residual is the square root of a ratio of sums and loses
    most last-bit changes of a sum: shape_cases.shell_seed holds seeds at which the one-trip sum shows here too; the
    solves below are the sensitive check of the sums.)"""
    p, div = C.stored_shell_pair(N, dtype, C.shell_seed(N))
    want = D.bits(R.poisson_residual(p, div))
    assert D.bits(residual_copy(p, div)) == want, "the copy is not the reference"
    dv = div[I, I, I].astype(F64)
    dd = R.tree_sum(dv * dv, dtype)
    assert D.bits(residual_copy(p, div, None, dd)) == want
    caught = {m: D.bits(residual_copy(p, div, m, dd)) != want for m in SHELLS + ["seam_hi", "seam_lo", "one_trip", "ragged"]}
    print(f"N={N} {C.dname(dtype)}: caught {' '.join(m for m, c in caught.items() if c)}")
    for m in SHELLS:
        assert caught[m], m
    assert caught["seam_hi"] == caught["seam_lo"] == two_trip(N, dtype)
    assert caught["one_trip"] == ((N, dtype) in ONE_TRIP_CAUGHT)
    assert caught["one_trip"] or (N, dtype) in ONE_TRIP_BLIND or not two_trip(N, dtype)
    assert caught["ragged"] == ragged(N, dtype)


def test_one_trip_tables_cover_every_two_trip_size():
    assert ONE_TRIP_CAUGHT | ONE_TRIP_BLIND == {s for s in RESIDUAL_SHAPES if two_trip(*s)}
    for dtype in C.DTYPES:
        W = D.vec_width(dtype)
        sizes = {N for N, t in C.CG_SHAPES if t == dtype}
        assert {N % W for N in sizes if N > W} == set(range(W))  # every residue, beyond the all-wall sizes
        assert {64 * W, 64 * W + 1} <= sizes  # no second trip; a second trip of one ragged vector
        assert any(64 * W + W < N < 64 * W + 2 * W and N % W for N in sizes)  # a full vector and a ragged one
        assert any(N > 64 * W + 8 * W for N in sizes)  # a second trip of many lanes
        assert 3 in {N % 4 for N in sizes if N > 3}


ZERO_COLUMN = [(5, np.float32), (13, np.float64), (70, np.float32), (131, np.float64)]


@pytest.mark.parametrize("N,dtype", ZERO_COLUMN, ids=[sid(s) for s in ZERO_COLUMN])
def test_the_shell_column_sum_is_the_reference_on_a_zero_column(N, dtype):
    """The ragged path of tree_sum_with_shell_column (N mod W != 0) with +0.0 in the shell column: the reference's bits."""
    assert ragged(N, dtype)
    terms = np.zeros((N, N, N + 1), F64)
    terms[:, :, :N] = C.decades_field(N, dtype, N)[I, I, I].astype(F64) ** 2
    assert D.bits(tree_sum_with_shell_column(terms, dtype)) == D.bits(R.tree_sum(np.ascontiguousarray(terms[:, :, :N]), dtype))


# ---- (b) the solve stopped by max_iters ----------------------------------------------------------------------------
def checked_reference(monkeypatch, u, v, w, tol, max_iters, blind, blind_sum=False, differ=(), only=None):
    """R.project_cg, and on every field it puts under the stencil the mutants `blind` return the reference's bits: a
    mutant whose every application equals the reference's is the reference on the whole run. (`only`: the applications
    that are compared, all if None — above N = 130 the first and the last, each comparison there costing as much as an
    iteration; that d has its mirror shells on every application in between is the same line of the SPEC.) With blind_sum the same for
    the one-trip sum on every set of terms the run sums. The mutants `differ` must change q on every application (used
    above N = 200 in place of a mutated run, which takes 10 to 15 s there: a q that differs in the first iteration
    changes r, and every number after it)."""
    calls = []

    def tree_sum(terms, dtype, slabs=1):
        want = true_tree_sum(terms, dtype, slabs)
        assert D.bits(tree_sum_one_trip(terms, dtype)) == D.bits(want), "one_trip differs"
        return want

    true_tree_sum = R.tree_sum
    if blind_sum:
        monkeypatch.setattr(R, "tree_sum", tree_sum)

    def apply_A(x):
        want = true_apply_A(x)
        for m in blind if only is None or len(calls) in only else ():
            assert same_bits(apply_A_mut(x, m), want), f"{m} differs on application {len(calls)}"
        for m in differ:
            assert not same_bits(apply_A_mut(x, m), want), f"{m} is the reference on application {len(calls)}"
        calls.append(1)
        return want

    true_apply_A = R.apply_A
    monkeypatch.setattr(R, "apply_A", apply_A)
    try:
        return R.project_cg(u, v, w, tol, max_iters), len(calls)
    finally:
        monkeypatch.setattr(R, "apply_A", true_apply_A)
        monkeypatch.setattr(R, "tree_sum", true_tree_sum)


SCALAR_MUTANTS = ["alpha_double", "beta_double", "t_products", "mu_zero", "mu_in_T", "no_set_bnd"]
SCALAR_SIZES = [5, 13, 31, 34, 64, 65, 70]  # (N <= 3: printed, not asserted; N = 1 has r = 0 and no iteration)
SOLVE_SHAPES = C.CG_SHAPES


@pytest.mark.parametrize("N,dtype", SOLVE_SHAPES, ids=[sid(s) for s in SOLVE_SHAPES])
def test_solves_tell_the_mutants(N, dtype, monkeypatch):
    """project_cg on cg_velocity at max_iters = cg_iters(N), the reference reporting MAX_ITERS.
    * No shell mutant can show: d has been through set_bnd(0, .) whenever the stencil reads it (finding 1 of the issue
      behind this file) — every application is compared. The same for the seam mutants at one-trip sizes.
    * seam_lo is caught at every two-trip size; seam_hi at every two-trip size but N = 64 W + 1, where the cell it takes,
      x[N+1], mirrors the right one, x[N] (only (a) sees it there). The one-trip sum is caught at 200 / 131 (fp64); at
      130 / 129 and 257 every sum of the run is compared and has the reference's bits. In fp32 the solve on this input
      does not see the order at all (262 and 324: left to (a)): alpha and beta are rounded to T, and rel_residual came
      out in the reference's bits too at the seeds tried — products of fp32 numbers are exact in double, and a lane's
      few additions of terms of one magnitude are exact as well. So on the GPU the second-trip order of the fp32 sums
      is checked through poisson_residual only, which shares cg_apply_dot's sum but not cg_update's.
    * Sizes 5 .. 70: alpha or beta kept in double and products formed in T are caught in fp32 and are the reference in
      fp64 (the same expressions); mu = 0 and the skipped set_bnd are caught in both; mu divided in T is the reference
      in fp64 (the same division) and at N = 64 (N^3 a power of two: either division only changes the exponent). One
      ulp of mu reaches r only where it flips the rounding of div - mu in some cell (about one seed in three):
      shape_cases.CG_SEEDS holds a seed that does at every size from 5 to 70 but 64."""
    u, v, w = C.cg_velocity(N, dtype, C.cg_seed(N))
    iters = C.cg_iters(N)
    two = two_trip(N, dtype)
    f32 = dtype == np.float32
    want, applications = checked_reference(monkeypatch, u, v, w, TOL, iters,
                                           SHELLS + ([] if two else ["seam_hi", "seam_lo"]), (N, dtype) in ONE_TRIP_BLIND,
                                           [m for m in ("seam_lo", "seam_hi") if two and N > 200
                                            and (m == "seam_lo" or N != D.LANES * D.vec_width(dtype) + 1)],
                                           None if N <= 130 else {0, iters - 1})
    if N >= 5:  # (N <= 3: at most 27 cells, solved exactly within the 8 iterations: CONVERGED)
        assert (want["status"], want["iterations"]) == (R.MAX_ITERS, iters) and applications == iters
    if N <= 200:
        assert same_outcome(cg_copy(u, v, w, TOL, iters), want), "the copy is not the reference"
    muts = []
    if two and N <= 200:
        muts += ["seam_hi", "seam_lo"] + (["one_trip"] if (N, dtype) in ONE_TRIP_CAUGHT and not f32 else [])
    if N <= 70:
        muts += SCALAR_MUTANTS
    caught = {m: not same_outcome(cg_copy(u, v, w, TOL, iters, m), want) for m in muts}
    print(f"N={N} {C.dname(dtype)}: caught {' '.join(m for m, c in caught.items() if c) or 'nothing'}")
    if two and N <= 200:
        assert caught["seam_lo"] and caught["seam_hi"] == (N != D.LANES * D.vec_width(dtype) + 1)
        assert caught.get("one_trip", True)
    if N <= 70 and not f32:
        assert not (caught["alpha_double"] or caught["beta_double"] or caught["t_products"] or caught["mu_in_T"])
    if N in SCALAR_SIZES:
        assert caught["mu_zero"] and caught["no_set_bnd"]
        if f32:
            assert caught["alpha_double"] and caught["beta_double"] and caught["t_products"]
            assert caught["mu_in_T"] == (N != 64)


# ---- (c) the long runs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
@pytest.mark.parametrize("N,iterations", LONG, ids=[f"N{n}" for n, _ in LONG])
def test_long_runs_converge_late_and_tell_the_scalar_mutants(N, iterations, dtype):
    """cg_velocity at seed 2, tol = 1e-3: CONVERGED after 83 / 113 / 127 iterations (at least 50: an input that converges
    early checks neither the rounding of alpha and beta over a long run nor the iteration the stop falls on). Over that
    many iterations a scalar kept in double changes the iteration count or the fields in fp32.

    sqrt_stop: no input here separates it. The two tests differ only where rho' / rho0 lies within a rounding of tol^2;
    over the histories of all six runs the two predicates agree at every iteration (asserted), so this mutant is the
    reference on every case of the GPU file. It is listed to say so."""
    u, v, w = C.cg_velocity(N, dtype, LONG_SEED)
    hist = []
    want = R.project_cg(u, v, w, TOL, LONG_MAX, history=hist)
    print(f"N={N} {C.dname(dtype)}: status {want['status']} iterations {want['iterations']} rel {want['rel_residual']!r}")
    assert want["status"] == R.CONVERGED and want["iterations"] >= 50
    assert want["iterations"] == iterations
    u0, v0, w0 = (f.copy() for f in (u, v, w))
    p, div = R.divergence(u0, v0, w0)
    s = R.tree_sum(div[I, I, I].astype(F64), dtype)
    r = div[I, I, I] - dtype(s / float(N) ** 3)
    rho0 = R.dot(r, r, dtype)
    for n, rho in enumerate(hist):
        assert (math.sqrt(rho / rho0) <= TOL) == (rho <= (TOL * TOL) * rho0), f"sqrt_stop differs at iteration {n + 1}"
    assert same_outcome(cg_copy(u, v, w, TOL, LONG_MAX), want), "the copy is not the reference"
    if dtype == np.float32:
        for m in ("alpha_double", "beta_double"):
            assert not same_outcome(cg_copy(u, v, w, TOL, LONG_MAX, m), want), m
