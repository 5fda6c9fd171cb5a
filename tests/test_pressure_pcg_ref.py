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
  shallow_r      slab emulation: r beyond a slab is current on the first plane only and stale on the planes beyond it
                 (an exchange of r that ships one plane where a pass of three or four sweeps reads two or three)
  stale_z        slab emulation: after a pass the iterate's ghost planes are not exchanged — the exchange ships the
                 partner buffer — so the next pass reads, beyond the slab, the iterate of two passes before (+0 at the
                 start of an M)
The slab emulation runs the passes it is given: the sweep counts of a case's plan in pcg_cases.PLANS. With everything
current ("emulated") it is the reference. The table test at the end shows that PLANS covers every pass kind.
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


SLAB_MUTANTS = ("stale_r", "shallow_r", "stale_z", "emulated")


def pcg_copy(u, v, w, tol, max_iters, m, mut=None, slabs=1, passes=None):
    """pressure_pcg_ref.project_cg (m >= 1) with mutation `mut` (None: the reference, line by line). passes: the sweep
    counts of the fused passes the slab emulation runs (default passes_of(m))."""
    assert passes is None or sum(passes) == m
    dtype = u.dtype
    T = dtype.type
    N = u.shape[0] - 2
    state = {"z": np.zeros((N + 2,) * 3, dtype), "r_old": np.zeros((N,) * 3, dtype)}

    def precondition(r):
        rhs = np.zeros((N + 2,) * 3, dtype)
        rhs[I, I, I] = r
        z0 = state["z"] if mut == "z_not_zeroed" else np.zeros_like(rhs)
        if mut in SLAB_MUTANTS:
            nzl = N // slabs
            stale = np.zeros_like(rhs)
            stale[I, I, I] = state["r_old"]
            z, older = z0, np.zeros_like(rhs)  # the iterate, and the iterate of the pass before
            for s in passes or passes_of(m):
                nxt = np.zeros_like(z)
                for g in range(slabs):
                    a, b = 1 + g * nzl, 1 + (g + 1) * nzl  # the slab's planes [a, b)
                    lo, hi = (0 if g == 0 else a), (N + 2 if g == slabs - 1 else b)  # wall slabs own the shell planes
                    seen, zseen = rhs, z
                    if mut in ("stale_r", "shallow_r"):
                        seen = stale.copy()
                        seen[a:b] = rhs[a:b]
                        if mut == "shallow_r":
                            seen[a - 1], seen[b] = rhs[a - 1], rhs[b]
                    if mut == "stale_z":
                        zseen = older.copy()
                        zseen[lo:hi] = z[lo:hi]
                    nxt[lo:hi] = sweeps(zseen, seen, s)[lo:hi]
                older, z = z, nxt
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


# ---- the pass plans (pcg_cases.PLANS) --------------------------------------------------------------------------------
def sweeps_of(plan):
    return [s for s, _, _ in PC.parse_plan(plan)]


# the slab cases of the GPU file the mutants are run on: every plan at N = 40 (two slabs of 20 planes), and one of the
# longest plans of each other (N, P); fp64 at 40 and 72 / 3, fp32 elsewhere
def mutant_cases():
    out = [c for c in PC.ON_SLABS if c.N == 40 and c.dtype == np.float64 and "SF_ZERO_SKIP" not in c.env]
    for N, P, m, dtype in ((64, 2, 12, np.float32), (64, 4, 12, np.float32), (72, 2, 10, np.float32), (72, 3, 10, np.float64)):
        out += [c for c in PC.ON_SLABS if (c.N, c.P, c.m, c.dtype) == (N, P, m, dtype)]
    return out


MUTANT_CASES = mutant_cases()


@pytest.mark.parametrize("case", MUTANT_CASES, ids=[c.id for c in MUTANT_CASES])
def test_plan_inputs_tell_shallow_r_and_stale_z(case):
    """Six iterations of cg_velocity, as tests/test_pressure_pcg_plans_gpu.py runs them, with the passes of the case's
    plan. The emulation with everything current is the reference. stale_z differs wherever there is a second pass;
    shallow_r differs wherever a pass has three or four sweeps, and is the reference where every pass has at most two
    (such a pass reads r on one plane beyond the slab): the control, as m = 1 is for stale_r."""
    assert len(MUTANT_CASES) == 12
    u, v, w = C.cg_velocity(case.N, case.dtype, PC.seed(case.N))
    passes = sweeps_of(case.plan)
    want = Q.project_cg(u, v, w, PC.TOL, PC.DECOMPOSED_ITERS, case.m)
    run = lambda mut: pcg_copy(u, v, w, PC.TOL, PC.DECOMPOSED_ITERS, case.m, mut, slabs=case.P, passes=passes)  # noqa: E731
    assert same_outcome(run("emulated"), want), "the slab emulation is not the reference"
    assert len(passes) >= 2 and not same_outcome(run("stale_z"), want)
    assert not same_outcome(run("stale_r"), want)
    assert same_outcome(run("shallow_r"), want) == (max(passes) <= 2), passes


def test_one_pass_cannot_show_stale_z():
    """m = 2 is one pass on the zero iterate: nothing of z is read beyond a slab."""
    u, v, w = C.cg_velocity(40, np.float32, PC.seed(40))
    assert same_outcome(pcg_copy(u, v, w, PC.TOL, 6, 2, "stale_z", slabs=2, passes=[2]), Q.project_cg(u, v, w, PC.TOL, 6, 2))


def test_the_mutant_cases_hold_both_kinds_of_plan():
    deep = [c for c in MUTANT_CASES if max(sweeps_of(c.plan)) >= 3]
    assert len(deep) >= 8 and len(MUTANT_CASES) - len(deep) >= 2  # (40 / 2 m = 3 and 64 / 4: pairs and singles only)


ONE_SLAB_PLANS = {2: "2Z", 5: "2Z 3", 6: "2Z 4", 7: "4Z 3", 8: "4Z 4", 9: "4Z 3 2", 10: "4Z 3 3", 11: "4Z 4 3", 12: "4Z 4 4"}
SLAB_PLANS = {  # (N, P, MARCH_MINP=4?) -> {m: plan}
    (72, 2, False): {5: "2Z 3+3", 7: "4Z 3+4", 8: "4Z 4+4", 9: "4Z 3+4 2", 10: "4Z 3+4 3+7", 11: "4Z 4+4 3+8", 12: "4Z 4+4 4+8"},
    (64, 2, False): {5: "2Z 3+3", 7: "4Z 3+4", 8: "4Z 4+4", 9: "4Z 3+4 2"},
    (64, 2, True): {10: "4Z 3+4 3+7", 11: "4Z 4+4 3+8", 12: "4Z 4+4 4+8"},
    (40, 2, False): {3: "2Z 1", 5: "2Z 3", 7: "4Z 3", 8: "4Z 4", 9: "4Z 3 2", 10: "4Z 3 3", 11: "4Z 4 3", 12: "4Z 4 4"},
    (72, 3, True): {7: "4Z 3+4", 8: "4Z 4+4", 10: "4Z 3+4 3", 12: "4Z 4+4 4"},
    (64, 4, False): {8: "2Z 2+2 2+4 2", 9: "2Z 2+2 2+4 2 1", 12: "2Z 2+2 2+4 2 2+2 2+4"},
}


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_the_plan_table_is_the_one_written_down(dtype):
    """The plans of pcg_cases.PLANS (its model of plan_solve) against the table as it stands in docs/NEXT.md, which the
    GPU file confirmed from the traces: a change of the model, or of the cases, shows here first."""
    got_one, got_slabs = {}, {}
    for c in PC.PLANS:
        if c.dtype != dtype or "SF_ZERO_SKIP" in c.env or c.tuned:
            continue
        assert c.env.get("SF_MARCH_MINCELLS_K") == "0"
        if c.P == 1:
            assert c.G == 1
            if c.m in ONE_SLAB_PLANS:
                got_one.setdefault(c.N, {})[c.m] = c.plan
        else:
            assert c.G == (2 if (c.N, c.P) == (64, 4) else 4)
            got_slabs.setdefault((c.N, c.P, "SF_MARCH_MINP" in c.env), {})[c.m] = c.plan
    assert got_one == {40: ONE_SLAB_PLANS, 64: ONE_SLAB_PLANS}
    assert got_slabs == SLAB_PLANS
    # the rccl-self cases that grow say SF_TRAP=5 (such a context's default is 0 or what it measures), the copy cases
    # say nothing; both transports occur at every (N, P)
    for c in PC.ON_SLABS:
        if not c.tuned:
            assert ("SF_TRAP" in c.env) == (c.transport == "rccl-self" and "+" in c.plan), c.id
    for key in {(c.N, c.P) for c in PC.ON_SLABS}:
        assert {c.transport for c in PC.ON_SLABS if (c.N, c.P) == key} == {"copy", "rccl-self"}
    assert sum(c.tuned for c in PC.PLANS) == 2
    # what the issue's other statements about the model come to
    assert PC.model(40, np.float64, 2, 8, dict(PC.MARCH, SF_GHOST="3")) == (3, "2Z 3 3")
    assert PC.model(40, dtype, 1, 8, PC.NO_SKIP) == (1, "4C 4")
    assert PC.model(34, np.float32, 2, 4) == (1, "1C 1 1 1") and PC.model(34, np.float64, 2, 4) == (2, "2Z 2+2")


@pytest.mark.parametrize("slabs", [False, True], ids=["one-slab", "slabs"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_the_plan_table_covers_every_pass_kind(dtype, slabs):
    """In each precision, on one slab and on slabs: passes of 1, 2, 3 and 4 sweeps; a first pass on the implicit zero
    and one on the stored zero, of two and of four sweeps each; a four-sweep pass followed by a three-sweep one; and on
    slabs a grown pass, a pass that snaps back after a grown one, a second block in one solve, and the growth of a 3
    after a 4 by max(S_j, S_j-1) = 4. One slab has no boundary launch: no plan grows there."""
    plans = [PC.parse_plan(c.plan) for c in PC.PLANS if c.dtype == dtype and (c.P > 1) == slabs and not c.tuned]
    passes = [p for plan in plans for p in plan]
    pairs = [(a, b) for plan in plans for a, b in zip(plan, plan[1:])]
    assert {s for s, _, _ in passes} == {1, 2, 3, 4}
    assert {(s, f) for s, f, _ in passes if f} >= {(2, "Z"), (4, "Z"), (2, "C"), (4, "C")}
    assert any(a[0] == 4 and b[0] == 3 for a, b in pairs)
    grown = [p for p in passes if p[2]]
    if not slabs:
        assert not grown and (1, "C", 0) in passes
        return
    assert {s for s, _, _ in grown} == {2, 3, 4}
    assert any(a[2] and not b[2] for a, b in pairs), "no pass snaps back after a grown one"
    assert any(a[2] and b[2] > a[2] for a, b in pairs), "no block of three passes"
    assert any([bool(e) for _, _, e in plan] == [False, True, True, False, True, True] for plan in plans), "no second block"
    assert any(a[0] == 4 and b[0] == 3 and b[2] == 4 for a, b in pairs)
