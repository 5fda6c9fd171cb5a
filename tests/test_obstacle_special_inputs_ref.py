"""The inputs of tests/test_obstacle_special_gpu.py, checked on the CPU (tests/obstacle_special_cases.py holds both
files' cases):

* with their default arguments the hooks of the masked numpy references (`ops`, and the names of SPECIAL_WRONG for
  `wrong`) change no bit: digests of results that the references gave on merged inputs before they had any hook;
* every wrong reading the hooks can switch to - ClampMinMax, Flush, FaceMinus, SkipZeroWeight, solid_as_product,
  replace_as_blend, first_smooth_no_zero, grad_add - changes the result of a named case of the GPU file, while the merged
  inputs of §17 (tests/obstacle_transport_cases.py) tell none of the first four from the reference;
* the conditions under which a case compares what it is meant to hold on the reference for every GPU case: every kind of
  special value sits in a fluid cell with a closed face, the b = 0 advect has a fluid cell with -0 and +-inf of its own
  standing in for a solid sample, the landing cells land, and no compared field drowns in NaN."""
import hashlib

import numpy as np
import pytest

import obstacle_cases as OC
import obstacle_mg_cases as MC
import obstacle_special_cases as SP
import obstacle_transport_cases as TC
import obstacle_transport_ref as TR
import obstacles_mg_ref as OM
import obstacles_ref as OB
import shape_cases as C
import stable_cases as SC
import stable_ref as S3
from gpu_support import DIFF, DT, VISC, random_fields
from ref_support import same_bits
from shape_cases import dname

I = SP.I
F32, F64 = np.float32, np.float64


# ---- the default hooks change no bit ---------------------------------------------------------------------------------
def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def solve_digest(w):
    return digest(w["u"], w["v"], w["w"], w["p"], w["div"], np.array([w["status"], w["iterations"]]),
                  np.array([w["rel_residual"]]))


def _diffuse(fam, N, t, b, K):
    x, x0 = TC.fields(fam, N, t, b)
    TR.diffuse_masked(b, x, x0, TC.DIFF, DT, K, OC.mask(fam, N, t))
    return digest(x)


def _advect(fam, N, t, b):
    d0 = TC.fields(fam, N, t, b)[1]
    d = np.zeros_like(d0)
    TR.advect_masked(b, d, d0, *TC.velocity(fam, N, t), DT, OC.mask(fam, N, t))
    return digest(d)


def _project(fam, N, t, m):
    return solve_digest(OB.project_cg(*C.cg_velocity(N, t, OC.seed(fam, N) + 5000), OC.mask(fam, N, t), OC.TOL, OC.ITERS, m))


def _vcycle(fam, N, t, s):
    r = MC.rhs_fields(fam, N, t)[1]
    return digest(OM.vcycle(r[I], MC.mask(fam, N, t), *s))


def _mg_project(fam, N, t):
    return solve_digest(OM.project_cg(*MC.velocity(fam, N, t), MC.mask(fam, N, t), MC.TOL, 4, *MC.DEFAULT))


def _step(N, t):
    f = random_fields(N, t, 177)
    mask = OC.mask("box", N, t)
    vel = TR.vel_step(f, mask, 4, DT, VISC, lambda u, v, w: OB.project_cg(u, v, w, mask, 1e-2, 10, 0))
    dens = TR.dens_step(f["dens"], f["dens0"], vel["u"], vel["v"], vel["w"], mask, 4, DT, DIFF)
    return digest(vel["u"], vel["v"], vel["w"], dens)


# (the call on merged inputs, the digest of its result at the commit before the references took `ops`)
BEFORE_THE_HOOKS = [
    (_diffuse, ("box", 13, F32, 1, 2), "a49f7f9fdac358ef"),
    (_diffuse, ("random30", 34, F64, 0, 5), "79417e65fa7e3802"),
    (_diffuse, ("walls", 13, F64, 3, 1), "5c56a15618596383"),
    (_diffuse, ("special", 13, F32, 2, 2), "f7112cf6e2704a15"),
    (_advect, ("box", 13, F32, 0), "152b4fb63c220b67"),
    (_advect, ("walls", 34, F64, 2), "f3b6a3e85345428f"),
    (_advect, ("random30", 13, F64, 0), "5e8855c8ee6e28ea"),
    (_advect, ("special", 13, F32, 1), "ebef8d549484fa24"),
    (_project, ("random30", 13, F32, 0), "70e4621496cee881"),
    (_project, ("walls", 13, F64, 2), "90850ea8e84bd757"),
    (_project, ("box", 34, F32, 2), "49e17794d599a284"),
    (_project, ("special", 5, F64, 0), "aa3a0bf7b006b612"),
    (_vcycle, ("odd_box", 16, F32, MC.DEFAULT), "2ffe0d91c65244a0"),
    (_vcycle, ("random30", 12, F64, MC.DEFAULT), "0b1a258530c91105"),
    (_vcycle, ("walls", 34, F32, MC.SHORT), "a84b9d9ddbdf95d0"),
    (_vcycle, ("box", 13, F32, MC.DEFAULT), "aa5b18a34e543a3c"),
    (_mg_project, ("odd_box", 16, F32), "b3af5a2fb22ba5b1"),
    (_mg_project, ("walls", 34, F64), "edd3be818c0b978e"),
    (_step, (13, F64), "54e7a1bb9c8e9691"),
    (_step, (34, F32), "6b3c8e92548e3a1a"),
]


def _arg_id(a):
    return dname(a) if isinstance(a, type) else "-".join(map(str, a)) if isinstance(a, tuple) else str(a)


@pytest.mark.parametrize("call,args,want", BEFORE_THE_HOOKS,
                         ids=[call.__name__.strip("_") + "-" + "-".join(_arg_id(a) for a in args)
                              for call, args, _ in BEFORE_THE_HOOKS])
def test_the_default_hooks_change_no_bit(call, args, want):
    assert call(*args) == want


# ---- the wrong readings ------------------------------------------------------------------------------------------------
def differing(got, want):
    """{name: entries whose bits differ} over the fields of two results (dicts of arrays)."""
    out = {}
    for n in want:
        if isinstance(want[n], np.ndarray):
            uint = np.uint32 if want[n].dtype == np.float32 else np.uint64
            count = int((got[n].view(uint) != want[n].view(uint)).sum())
            if count:
                out[n] = count
    return out


def operators(family, mfam, N, t):
    return SP.operator_id(family, mfam, N, t), lambda wrong, ops: SP.operator_case(family, mfam, N, t, wrong, ops)


def landing(N, t):
    return SP.landing_id(N, t), lambda wrong, ops: SP.landing_case(N, t, wrong, ops)


def projection(kind, N, t, mfam, m=0):
    return SP.project_id(kind, N, t, mfam), lambda wrong, ops: SP.project_case(kind, N, t, mfam, m, wrong, ops)


def cycle(kind, N, t, s, mfam):
    return SP.cycle_id(kind, N, t, s, mfam), lambda wrong, ops: {"z": SP.cycle_case(kind, N, t, s, mfam, wrong)}


def step(N, t):
    def run(wrong, ops):
        vel, dens = SP.step_case(N, t, wrong, ops)
        return {"u": vel["u"], "v": vel["v"], "w": vel["w"], "dens": dens}
    return SP.step_id(N, t), run


# (wrong reading: a name of SPECIAL_WRONG or a class of TR.MUTANTS, (the id of a GPU case that tells it from the
# reference, how to run that case))
SEPARATES = [
    (TR.ClampMinMax, operators("specials", "box", 13, F32)),
    (TR.ClampMinMax, operators("specials", "walls", 34, F64)),
    (TR.Flush, operators("subnormal", "walls", 13, F32)),
    (TR.Flush, operators("subnormal", "random30", 34, F64)),
    (TR.FaceMinus, operators("zeros", "random30", 13, F32)),
    (TR.FaceMinus, operators("zeros", "walls", 34, F64)),
    (TR.FaceMinus, operators("specials", "box", 13, F64)),
    (TR.FaceMinus, projection("zeros", 13, F32, "random30")),
    (TR.FaceMinus, projection("zeros", 34, F32, "walls", 2)),
    (TR.SkipZeroWeight, landing(8, F32)),
    (TR.SkipZeroWeight, landing(64, F64)),
    (TR.SkipZeroWeight, operators("specials", "random30", 13, F64)),
    ("solid_as_product", operators("specials", "box", 13, F32)),
    ("solid_as_product", operators("subnormal", "random30", 5, F64)),
    ("solid_as_product", projection("subnormal", 13, F64, "walls")),
    ("replace_as_blend", operators("specials", "random30", 13, F32)),
    ("replace_as_blend", operators("zeros", "walls", 13, F64)),
    # (the steps are there for the shapes of the three-field forms; their data is finite and normal, and the solids
    # hold +0 after the first sweep, so of all the readings they see this one alone, by the sign of a zero)
    ("solid_as_product", step(34, F64)),
    ("first_smooth_no_zero", cycle("zeros", 34, F32, MC.SHORT, "odd_box")),
    ("grad_add", projection("zeros", 13, F64, "walls")),
    ("grad_add", projection("zero_region", 34, F64, "random30", 2)),
]


def reading_name(reading):
    return reading if isinstance(reading, str) else reading.__name__


def test_every_wrong_reading_has_a_case():
    named = {reading_name(r) for r, _ in SEPARATES}
    assert named == ({m.__name__ for m in TR.MUTANTS} | set(TR.SPECIAL_WRONG) | set(OB.SPECIAL_WRONG)
                     | set(OM.SPECIAL_WRONG))
    run = ({SP.operator_id(*c) for c in SP.OPERATORS} | {SP.landing_id(*c) for c in SP.LANDING}
           | {SP.project_id(k, *c) for k in SP.PROJECT_KINDS for c in SP.PROJECTIONS}
           | {SP.cycle_id(k, *c) for k in SP.CYCLE_KINDS for c in SP.CYCLES} | {SP.step_id(*c) for c in SP.STEPS})
    assert {case for _, (case, _) in SEPARATES} <= run  # (every named case is one the GPU file runs)


@pytest.mark.parametrize("reading,case", SEPARATES, ids=[f"{reading_name(r)}-{c[0]}" for r, c in SEPARATES])
def test_a_named_case_separates_each_wrong_reading(reading, case):
    name, run = case
    wrong, ops = (reading, S3.SPEC) if isinstance(reading, str) else (None, reading())
    differ = differing(run(wrong, ops), run(None, S3.SPEC))
    print(f"{reading_name(reading)} on {name}: entries that differ: {differ}")
    assert differ, f"{name} does not tell {reading_name(reading)} from the reference"


@pytest.mark.parametrize("mutant", TR.MUTANTS, ids=lambda m: m.__name__)
def test_the_merged_inputs_tell_no_mutant_from_the_reference(mutant):
    """What the cases above are for: on the normal, finite fields of tests/obstacle_transport_cases.py (N = 13 fp32 and
    N = 34 fp64 under box, random30 and walls) the clamps as min / max, flushed subnormals, effn as T(0) - x and a skipped
    zero-weight sample leave every bit of the §17 operators as it is."""
    for N, t in ((13, F32), (34, F64)):
        for fam in ("box", "random30", "walls"):
            mask = OC.mask(fam, N, t)
            for b in (0, 2):
                out = []
                for ops in (S3.SPEC, mutant()):
                    x, x0 = TC.fields(fam, N, t, b)
                    TR.diffuse_masked(b, x, x0, TC.DIFF, DT, 2, mask, ops=ops)
                    d = np.zeros_like(x0)
                    TR.advect_masked(b, d, x0, *TC.velocity(fam, N, t), DT, mask, ops=ops)
                    out.append((x, d))
                assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]), (fam, N, b)


def test_an_unseparated_sign_of_the_subnormal_cycle():
    """first_smooth_no_zero differs from §16 only where c_s r is -0 in a fluid cell, and then only in the sign of a zero,
    which the z + ... of a later sweep or of the prolongation can absorb. With r among the subnormals (c_s r underflows
    to -0 in some fluid cell of every case: test_conditions_hold_on_the_cycles) it is absorbed everywhere in all four
    cases - asserted here, so that nobody takes the subnormal cycles for a check of that rule. The all-zero r of the
    `zeros` kind, where whole neighbourhoods are -0, is what tells the two apart (SEPARATES)."""
    for N, t, s, mfam in SP.CYCLES:
        assert same_bits(SP.cycle_case("subnormal", N, t, s, mfam, "first_smooth_no_zero"),
                         SP.cycle_case("subnormal", N, t, s, mfam))


# ---- the conditions of every GPU case ------------------------------------------------------------------------------------
def check_operator_inputs(family, mfam, mask, one_plane=False):
    """The conditions of obstacle_special_cases on the inputs of one single-operator case."""
    N, dtype = mask.shape[0] - 2, mask.dtype.type
    near = SP.closed_fluid(mask)
    assert near.any()
    for b in TC.BS:
        K = SP.sweeps(N, b)
        assert K <= 4
        x, x0, nf = SP.sweep_inputs(family, mask, b, K)
        d0, u, v, w, nf_adv = SP.advect_inputs(family, mfam, mask, b, one_plane)
        if family == "specials":
            assert nf == SC.nonfinite_at(N, K) and nf_adv == SC.nonfinite_at(N)
            assert not SP.missing_kinds(x, near, nf) and not SP.missing_kinds(x0, near, nf)
            assert not SP.missing_kinds(d0, near, nf_adv)
            hit = SP.solid_sample(mask, (u, v, w))[0]
            for val in (-0.0, np.inf, -np.inf) if nf_adv else (-0.0,):
                assert (SP.is_kind(d0[I], val) & hit).any(), f"no fluid cell with {val} and a solid sample"
            if one_plane:
                assert all(np.isfinite(c).all() for c in (u, v, w))
                assert float(np.abs(dtype(DT) * dtype(N) * w).max()) < 1
        elif family == "zeros":
            on_axis = SP.closed_fluid(mask, b)
            assert not x0.any() and np.signbit(x0).all() and not x.any()
            assert on_axis.any() and (np.signbit(x[I]) == ~on_axis).all()
        else:
            tiny = np.finfo(dtype).tiny
            for f in (x, x0, d0):
                assert ((np.abs(f[I]) < tiny) & (f[I] != 0) & OB.Mask(mask).fluid).any()


@pytest.mark.parametrize("family,mfam,N,dtype", SP.OPERATORS, ids=[SP.operator_id(*c) for c in SP.OPERATORS])
def test_conditions_hold(family, mfam, N, dtype):
    mask = OC.mask(mfam, N, dtype)
    check_operator_inputs(family, mfam, mask)
    share = SP.check_nan_share(SP.operator_case(family, mfam, N, dtype), mask, SP.operator_id(family, mfam, N, dtype))
    print(f"{SP.operator_id(family, mfam, N, dtype)}: NaN on at most {share:.4f} of the fluid cells of a compared field")
    if family != "specials" or not SC.nonfinite_at(N):
        assert share == 0


@pytest.mark.parametrize("N,dtype", SP.SECOND_TRIP, ids=[f"N{n}-{dname(t)}" for n, t in SP.SECOND_TRIP])
def test_conditions_hold_at_the_second_trip(N, dtype):
    mask = OC.mask("walls", N, dtype)
    b = N % 4
    x, x0, nf = SP.sweep_inputs("specials", mask, b, 1)
    s = 64 * (16 // np.dtype(dtype).itemsize)
    assert nf and C.second_trip(N, dtype) and s + 1 <= N
    for f in (x, x0):
        assert not SP.missing_kinds(f, SP.closed_fluid(mask), nf)
        for val in C.SPECIALS:  # (one field's cell may take a later value; each kind stays on one of the two)
            assert SP.is_kind(f[1:-1, 1:-1, s], val).any() or SP.is_kind(f[1:-1, 1:-1, s + 1], val).any()
    share = SP.check_nan_share(SP.second_trip_case(N, dtype), mask, f"second trip N={N}")
    print(f"N={N}: NaN share {share:.5f}")


@pytest.mark.parametrize("N,P,transport,dtype", SP.DECOMPOSED, ids=[f"N{n}-P{p}-{tr}" for n, p, tr, _ in SP.DECOMPOSED])
def test_conditions_hold_on_the_decomposed_case(N, P, transport, dtype):
    mask, lin, adv, vel = SP.decomposed_inputs(N, P, dtype)
    check_operator_inputs("specials", "walls", mask, one_plane=True)
    fluid = OB.Mask(mask).fluid
    for b in TC.BS:
        for f in (lin[b][0], lin[b][1], adv[b]):
            for k in (N // P, N // P + 1):
                for val in C.SPECIALS:
                    assert (SP.is_kind(f[k, 1:-1, 1:-1], val) & fluid[k - 1]).any()
    SP.check_nan_share(SP.decomposed_case(N, P, dtype), mask, f"decomposed N={N} P={P}")


@pytest.mark.parametrize("N,dtype", SP.LANDING, ids=[SP.landing_id(*c) for c in SP.LANDING])
def test_conditions_hold_on_the_landings(N, dtype):
    mask, d0, u, v, w, cells = SP.landing_inputs(N, dtype)
    assert len(cells) == 3 and len(set(cells)) == 3
    hit, (s1, t1, r1) = SP.solid_sample(mask, (u, v, w), C.LANDING_DT, skip_first=True)
    for c, val in zip(cells, SP.LANDED):
        assert hit[c] and s1[c] == 0 and t1[c] == 0 and r1[c] == 0 and SP.is_kind(d0[I], val)[c]
    want = SP.landing_case(N, dtype)
    got = want["advect", 0][I]
    assert np.isnan(got[cells[0]]) and np.isnan(got[cells[1]])  # 0 * (+-inf), the weight of the solid sample
    SP.check_nan_share(want, mask, f"landing N={N}")


@pytest.mark.parametrize("N,dtype,mfam", SP.PROJECTIONS, ids=[f"{m}-N{n}-{dname(t)}" for n, t, m in SP.PROJECTIONS])
def test_conditions_hold_on_the_projections(N, dtype, mfam):
    mask = OC.mask(mfam, N, dtype)
    for kind in SP.PROJECT_KINDS:
        u, v, w = SP.project_velocity(kind, mask)
        if kind == "zeros":
            for axis, x in ((1, u), (2, v), (3, w)):
                on_axis = SP.closed_fluid(mask, axis)
                assert not x.any() and on_axis.any() and (np.signbit(x[I]) == ~on_axis).all()
        for m in (0, SP.PROJECT_SWEEPS):
            want = SP.project_case(kind, N, dtype, mfam, m)
            print(f"{kind} {mfam} N={N} m={m}: status {want['status']} iterations {want['iterations']}")
            SP.check_nan_share({n: want[n] for n in ("u", "v", "w", "p", "div")}, mask, f"{kind} N={N}")
            if kind == "zeros":  # an all-zero divergence: rho0 = 0 is CONVERGED at once
                assert (want["status"], want["iterations"]) == (OB.CONVERGED, 0) and not want["div"].any()
            if kind == "zero_region":
                assert want["iterations"] == SP.PROJECT_ITERS


@pytest.mark.parametrize("N,dtype,s,mfam", SP.CYCLES, ids=[MC.case_id(n, t, m, s) for n, t, s, m in SP.CYCLES])
def test_conditions_hold_on_the_cycles(N, dtype, s, mfam):
    mask = MC.mask(mfam, N, dtype)
    fluid = OB.Mask(mask).fluid
    for kind in SP.CYCLE_KINDS:
        r = SP.cycle_rhs(kind, mask)
        z = SP.cycle_case(kind, N, dtype, s, mfam)
        assert not np.isnan(z).any()
        if kind == "zeros":
            assert not r.any() and (np.signbit(r[I]) & fluid).any() and (~np.signbit(r[I]) & fluid).any()
        else:
            cs = dtype(1.0 / 7.0)
            assert (SP.is_kind(cs * r[I], -0.0) & fluid).any()  # the product the first sweep adds T(0) to
            assert z.any()


@pytest.mark.parametrize("N,dtype", SP.STEPS, ids=[SP.step_id(*c) for c in SP.STEPS])
def test_conditions_hold_on_the_steps(N, dtype):
    mask = SP.step_mask(N, dtype)
    vel, dens = SP.step_case(N, dtype)
    fields = {"u": vel["u"], "v": vel["v"], "w": vel["w"], "dens": dens}
    assert SP.check_nan_share(fields, mask, f"step N={N}") == 0
    mk = OB.Mask(mask)
    print(f"step N={N} {dname(dtype)}: fluid {mk.n_fluid} of {N ** 3}, status {vel['status']} iterations {vel['iterations']}")
    if N >= 5:
        assert 0 < mk.n_fluid < N ** 3 and vel["iterations"] >= 1
        assert not dens[I][mk.solid].any() and dens[I][mk.fluid].any()
