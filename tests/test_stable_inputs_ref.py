"""The inputs of tests/test_stable_bits_gpu.py, checked on the CPU (tests/stable_cases.py holds both files' cases):

* tests/stable_ref.py, the numpy statement of docs/SPEC.md §3 and §6, equals the C++ oracle in bits (NaN in the same
  entries) on every input family at N = 1, 2, 3, 5, 13, 34, 64, 65. This pins the oracle as well: no optimisation of
  its build has folded an expression of the SPEC into a value-equal one.
* Eight mutants - plausible kernel errors written into subclasses of stable_ref.Ops, never into the library - each
  differ from the reference on a case that the GPU file runs; the test id names the case.
* No GPU case drowns in NaN (stable_cases.check_nan_share on the oracle's result of every case)."""
import numpy as np
import pytest

import oracle_lib as O
import shape_cases as C
import stable_cases as SC
import stable_ref as R
from gpu_support import DIFF, VISC, assert_same_bits
from ref_support import same_bits
from shape_cases import DT, DTYPES, dname

SIZES = [1, 2, 3, 5, 13, 34, 64, 65]
SHAPES = [(N, t) for N in SIZES for t in DTYPES]
IDS = [f"N{N}-{dname(t)}" for N, t in SHAPES]
K_AT = {1: 1, 2: 2, 3: 3, 5: 4, 13: 4, 34: 2, 64: 4, 65: 5}  # (N, K) pairs of SC.LIN_CASES


# ---- the operators in both statements ----------------------------------------------------------------------------
def both(ops=R.SPEC):
    """name -> (oracle, stable_ref with ops) with one signature each; arrays in place."""
    return {
        "add_source": (lambda x, s: O.add_source(x, s, x.dtype.type(DT)), lambda x, s: R.add_source(x, s, DT)),
        "set_bnd": (O.set_bnd, lambda b, x: R.set_bnd(b, x, ops)),
        "lin_solve": (lambda b, x, x0, K: O.lin_solve(b, x, x0, x.dtype.type(SC.A_LIN), x.dtype.type(SC.C_LIN), K),
                      lambda b, x, x0, K: R.lin_solve(b, x, x0, SC.A_LIN, SC.C_LIN, K, ops)),
        "advect": (lambda b, d, d0, u, v, w, dt: O.advect(b, d, d0, u, v, w, d.dtype.type(dt)),
                   lambda b, d, d0, u, v, w, dt: R.advect(b, d, d0, u, v, w, dt, ops)),
        "project": (O.project, lambda u, v, w, p, div, K: R.project(u, v, w, p, div, K, ops)),
    }


def run_pointwise(fn, name, N, dtype, family, b=0):
    x, s = SC.pointwise_inputs(N, dtype, family)
    fn(x, s) if name == "add_source" else fn(b, x)
    return {"x": x}


def run_lin(fn, N, dtype, family, K, b, inputs=None):
    x, x0 = inputs if inputs is not None else SC.lin_inputs(N, dtype, family, K)
    x, x0 = x.copy(), x0.copy()
    fn(b, x, x0, K)
    return {"x": x, "x0": x0}


def run_project(fn, N, dtype, K):
    f = SC.project_inputs(N, dtype, K)
    fn(f["u"], f["v"], f["w"], f["u0"], f["v0"], K)
    return f


def run_advect(fn, b, inputs, dt=DT):
    d0, u, v, w = inputs
    d = np.zeros_like(d0)
    fn(b, d, d0, u, v, w, dt)
    return {"d": d}


def run_tracers(advect, sample, N, dtype, exact=False):
    pos, f, dt = SC.tracer_inputs(N, dtype, exact)
    pos = pos.copy()
    for _ in range(3):
        advect(pos, f["u"], f["v"], f["w"], pos.dtype.type(dt))
    d, s = sample(pos, f["dens"], f["u"], f["v"], f["w"])
    return {"pos": pos, "dens": d, "speed": s}


def assert_same(got, want, what):
    for n in want:
        assert_same_bits(got[n], want[n], f"{what}: {n}", nan_ok=True)


# ---- stable_ref == oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", SC.FAMILIES)
@pytest.mark.parametrize("N,dtype", SHAPES, ids=IDS)
def test_pointwise_and_lin_solve_equal_the_oracle(N, dtype, family):
    o, r = both()
    assert_same(run_pointwise(r["add_source"], "add_source", N, dtype, family),
                run_pointwise(o["add_source"], "add_source", N, dtype, family), "add_source")
    for b in range(4):
        assert_same(run_pointwise(r["set_bnd"], "set_bnd", N, dtype, family, b),
                    run_pointwise(o["set_bnd"], "set_bnd", N, dtype, family, b), f"set_bnd b={b}")
        assert_same(run_lin(r["lin_solve"], N, dtype, family, K_AT[N], b),
                    run_lin(o["lin_solve"], N, dtype, family, K_AT[N], b), f"lin_solve b={b}")


both = (lambda f: lambda ops=R.SPEC: tuple({n: pair[q] for n, pair in f(ops).items()} for q in (0, 1)))(both)


@pytest.mark.parametrize("N,dtype", SHAPES, ids=IDS)
def test_project_advect_and_tracers_equal_the_oracle(N, dtype):
    o, r = both()
    for K in (0, 1, 2, 5):
        assert_same(run_project(r["project"], N, dtype, K), run_project(o["project"], N, dtype, K), f"project K={K}")
    inputs = SC.advect_inputs(N, dtype)
    for b in range(4):
        assert_same(run_advect(r["advect"], b, inputs), run_advect(o["advect"], b, inputs), f"advect b={b}")
    dt = C.LANDING_DT if N in (64,) else DT
    landing = C.exact_landing(N, dtype, N, dt)
    assert_same(run_advect(r["advect"], 1, landing, dt), run_advect(o["advect"], 1, landing, dt), "advect, exact landing")
    for exact in (False, True) if N == 64 else (False,):
        n = 16 if exact else N
        assert_same(run_tracers(R.tracers_advect, R.tracers_sample, n, dtype, exact),
                    run_tracers(O.tracers_advect, O.tracers_sample, n, dtype, exact), f"tracers exact={exact}")


# ---- the mutants ---------------------------------------------------------------------------------------------------
def flush(x):
    return np.where(np.abs(x) < np.finfo(x.dtype).tiny, x.dtype.type(0) * x, x)  # (to a zero of the same sign)


class ZeroFirst(R.Ops):  # 1: the zero-iterate first sweep as x0 * inv
    def sweep(self, x, x0, a, inv, it):
        return x0[R.I] * inv if it == 0 and not x.any() else super().sweep(x, x0, a, inv, it)


class FaceMinus(R.Ops):  # 2: a negated face as T(0) - x
    def face(self, s, v):
        return v.dtype.type(0) - v if s < 0 else s * v


class EdgeHalves(R.Ops):  # 3: an edge as half*A + half*B
    def edge(self, half, a, b):
        return half * a + half * b


class Flush(R.Ops):  # 4: subnormals flushed to zero on input and output of a sweep
    def sweep(self, x, x0, a, inv, it):
        return flush(super().sweep(flush(x), flush(x0), a, inv, it))


def hw_clamp(x, lo, hi):
    return np.fmax(lo, np.fmin(hi, x))  # a hardware min / max: a NaN operand is ignored


class ClampMinMax(R.Ops):  # 5: the advect clamps as fmax(lo, fmin(hi, x))
    def trace(self, vel, dt0):
        T = vel[0].dtype.type
        N = vel[0].shape[0] - 2
        idx, pos = [], []
        for ax, comp in enumerate(vel):
            shape = [1, 1, 1]
            shape[2 - ax] = N
            with np.errstate(invalid="ignore"):
                x = hw_clamp(np.arange(1, N + 1).astype(T).reshape(shape) - dt0 * comp[R.I], T(0.5), T(N) + T(0.5))
            idx.append(np.clip(x.astype(np.int64), 0, N))
            pos.append(x)
        return idx, pos


class SkipZeroWeight(R.Ops):  # 6: advect skips the i0 + 1 samples where s1 == 0
    def combine(self, s0, lo, s1, hi):
        return np.where(s1 == 0, s0 * lo, s0 * lo + s1 * hi)


class GradAdd(R.Ops):  # 7: project_sub as u + c_grad*(p[i-1] - p[i+1])
    def grad_sub(self, u, c_grad, pp, pm):
        return u + c_grad * (pm - pp)


class TracerMinMax(R.Ops):  # 8: tracers_advect clamping with NaN-ignoring min / max
    def clamp_coord(self, x, lo, hi):
        return hw_clamp(x, lo, hi)


def lin_case(N, K, dtype, family, b):
    return lambda fn: run_lin(fn["lin_solve"], N, dtype, family, K, b)


# (mutant, the case of the GPU file that tells it from the reference: its name and how to run it)
F32, F64 = np.float32, np.float64
MUTANTS = [
    (ZeroFirst, "project-N13-f32-K2", lambda fn: run_project(fn["project"], 13, F32, 2)),
    (ZeroFirst, "project-N64-f64-K8", lambda fn: run_project(fn["project"], 64, F64, 8)),
    (FaceMinus, "set_bnd-zeros-N5-f32-b1", lambda fn: run_pointwise(fn["set_bnd"], "set_bnd", 5, F32, "zeros", 1)),
    (FaceMinus, "lin_solve-zeros-N34-f64-K2-b3", lin_case(34, 2, F64, "zeros", 3)),
    (EdgeHalves, "set_bnd-subnormal-N13-f32-b0", lambda fn: run_pointwise(fn["set_bnd"], "set_bnd", 13, F32, "subnormal", 0)),
    (EdgeHalves, "set_bnd-subnormal-N64-f64-b2", lambda fn: run_pointwise(fn["set_bnd"], "set_bnd", 64, F64, "subnormal", 2)),
    (Flush, "lin_solve-subnormal-N13-f32-K4-b0", lin_case(13, 4, F32, "subnormal", 0)),
    (Flush, "lin_solve-subnormal-N65-f64-K5-b2", lin_case(65, 5, F64, "subnormal", 2)),
    (ClampMinMax, "advect-N13-f32-b0", lambda fn: run_advect(fn["advect"], 0, SC.advect_inputs(13, F32))),
    (ClampMinMax, "advect-N65-f64-b2", lambda fn: run_advect(fn["advect"], 2, SC.advect_inputs(65, F64))),
    (SkipZeroWeight, "advect-landing-N8-f32", lambda fn: run_advect(fn["advect"], 0, C.exact_landing(8, F32, 8), C.LANDING_DT)),
    (SkipZeroWeight, "advect-landing-N64-f64", lambda fn: run_advect(fn["advect"], 0, C.exact_landing(64, F64, 64), C.LANDING_DT)),
    (GradAdd, "project-N5-f32-K0", lambda fn: run_project(fn["project"], 5, F32, 0)),
    (GradAdd, "project-N34-f64-K8", lambda fn: run_project(fn["project"], 34, F64, 8)),
    (TracerMinMax, "tracers-N4-f32", None),
    (TracerMinMax, "tracers-N33-f64", None),
]


@pytest.mark.parametrize("mutant,case,run", MUTANTS, ids=[f"{m.__name__}-{c}" for m, c, _ in MUTANTS])
def test_a_gpu_case_tells_the_mutant_from_the_reference(mutant, case, run):
    ops = mutant()
    if run is None:
        N, dtype = int(case.split("-")[1][1:]), F32 if case.endswith("f32") else F64
        want = run_tracers(R.tracers_advect, R.tracers_sample, N, dtype)
        got = run_tracers(lambda *a: R.tracers_advect(*a, ops=ops), lambda *a: R.tracers_sample(*a, ops=ops), N, dtype)
    else:
        want, got = run(both()[1]), run(both(ops)[1])
    differing = [n for n in want if not same_bits(got[n], want[n])]
    print(f"{mutant.__name__} on {case}: differs in {differing}")
    assert differing, f"{case} does not tell {mutant.__name__} from the reference"


# ---- no GPU case drowns in NaN -------------------------------------------------------------------------------------
def test_nan_share_of_every_lin_solve_and_pointwise_case():
    o = both()[0]
    for dtype in DTYPES:
        for N in C.SIZES:
            for family in SC.FAMILIES:
                SC.check_nan_share(run_pointwise(o["add_source"], "add_source", N, dtype, family), f"add_source N={N}")
        for N, K in SC.LIN_CASES + [(n, k) for n, k, t in SC.LIN_BIG if t == dtype]:
            for family in SC.FAMILIES:
                SC.check_nan_share(run_lin(o["lin_solve"], N, dtype, family, K, 0), f"lin_solve {family} N={N} K={K}")
        x, x0, K = SC.lin_n5_nonfinite(dtype)
        want = run_lin(o["lin_solve"], 5, dtype, None, K, 0, (x, x0))
        SC.check_nan_share(want, "lin_solve N=5 with non-finite values")
        assert np.isnan(want["x"]).any()


def test_nan_share_of_every_advect_project_and_step_case():
    o = both()[0]
    for dtype in DTYPES:
        for N in C.SIZES + [n for n, t in SC.ADVECT_BIG if t == dtype]:
            SC.check_nan_share(run_advect(o["advect"], 0, SC.advect_inputs(N, dtype)), f"advect N={N}")
        for N, dt in SC.LANDING_CASES:
            SC.check_nan_share(run_advect(o["advect"], 0, C.exact_landing(N, dtype, N, dt), dt), f"landing N={N}")
        for N, P, transport in C.DECOMPOSED:
            SC.check_nan_share(run_advect(o["advect"], 0, SC.advect_inputs(N, dtype, True)), f"advect P={P} N={N}")
        for N, K in SC.PROJECT_CASES:
            SC.check_nan_share(run_project(o["project"], N, dtype, K), f"project N={N} K={K}")
        for N in (34, 64):
            f = SC.step_inputs(N, dtype, "random")
            src = {n: f[n].copy() for n in ("u0", "v0", "w0", "dens0")}
            for _ in range(2):
                for n in src:
                    f[n][...] = src[n]
                O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), SC.STEP_K)
            SC.check_nan_share(f, f"two steps N={N}")
            assert np.isnan(f["dens"]).any()
        for N in SC.TRACER_SIZES:
            SC.check_nan_share(run_tracers(O.tracers_advect, O.tracers_sample, N, dtype), f"tracers N={N}")
