"""External forces (docs/SPEC.md §8), MacCormack advection (§9) and reductions / diagnostics (§10) on the GPU at every
shape and in every kernel form: the sizes of tests/shape_cases.py (1, 2, 3; rows of less than a wave; one full wave; two
to four waves with a ragged tail; the second trip of the §10 row partial), the four values of SF_ADVECT_ROW for the
MacCormack kernels, traces of several cells that vary along a row, and the special values (NaN, infinities, signed
zeros, ties) the SPEC's select forms exist for. tests/test_shape_inputs_ref.py shows on the CPU that these inputs tell
a subtly wrong kernel from a right one.

Every comparison is exact bit equality (gpu_support.assert_same_bits) against the numpy references (maccormack_ref,
forces_ref, diagnostics_ref). Where an input holds NaN (nan_ok): the same entries NaN, every other entry the same bits.
References are computed once per (N, precision) and reused across the forms."""
import numpy as np
import pytest

import forces_ref as F
import maccormack_ref as M
import oracle_lib as O
import shape_cases as C
from gpu_support import (DIFF, DT, NAMES, STATE, USER, VISC, Cache, advect_form, assert_same_bits, check_diag,  # noqa: F401
                         check_reduce, make, set_forces)  # (advect_form: a fixture, parametrised indirectly below)

pytestmark = pytest.mark.gpu

SL, MC = M.SEMI_LAGRANGIAN, M.MACCORMACK
FORMS = ["default", "gather", "row", "pairs"]


# ---- §9: the operator in every form ------------------------------------------------------------------------------
_OPERATOR = Cache()


def operator_reference(N, dtype, one_plane=False):
    def build():
        u, v, w = (C.mixed_flow_one_plane if one_plane else C.mixed_flow)(N, dtype, N)
        d0 = C.normal_field(N, dtype, N)
        return d0, u, v, w, [M.advect_mc(b, np.zeros_like(d0), d0, u, v, w, DT) for b in range(4)]

    return _OPERATOR.get((N, C.dname(dtype), one_plane), build)


def run_operator(fs, d0, u, v, w, want, what, nan_ok=False):
    for n, a in (("dens0", d0), ("u", u), ("v", v), ("w", w)):
        fs.upload(n, a)
    for b in range(4):
        if want[b] is None:
            continue
        fs.upload("dens", np.full(d0.shape, 7.0, d0.dtype))
        fs.advect_maccormack(b, "dens", "dens0", "u", "v", "w")
        fs.sync()
        assert_same_bits(fs.download("dens"), want[b], f"{what} b={b}", nan_ok)
    for n, a in (("dens0", d0), ("u", u), ("v", v), ("w", w)):
        assert_same_bits(fs.download(n), a, f"{what}: input {n} after the operator", nan_ok)


MC_OPERATOR_CASES = [(N, t, form) for N, t in C.SHAPES for form in FORMS]


@pytest.mark.parametrize("N,dtype,advect_form", MC_OPERATOR_CASES, indirect=["advect_form"],
                         ids=[f"N{N}-{C.dname(t)}-{f}" for N, t, f in MC_OPERATOR_CASES])
def test_maccormack_operator(N, dtype, advect_form):
    """sf_advect_maccormack, b = 0..3, on mixed_flow (traces of up to 2.5 cells, a share of neighbouring cells landing
    in neighbouring cells and a share not, all three outcomes of §9) at P = 1."""
    d0, u, v, w, want = operator_reference(N, dtype)
    with make(N, dtype) as fs:
        run_operator(fs, d0, u, v, w, want, f"N={N} {advect_form}")


SLAB_CASES = [(N, P, tr, t, form) for N, P, tr in C.DECOMPOSED for t in C.DTYPES for form in ("default", "row")]


@pytest.mark.parametrize("N,P,transport,dtype,advect_form", SLAB_CASES, indirect=["advect_form"],
                         ids=[f"N{N}-P{P}-{tr}-{C.dname(t)}-{f}" for N, P, tr, t, f in SLAB_CASES])
def test_maccormack_operator_on_slabs(N, P, transport, dtype, advect_form):
    """The same with w scaled to |dt0 w| < 1 (one ghost plane); u and v still trace over cells."""
    d0, u, v, w, want = operator_reference(N, dtype, one_plane=True)
    with make(N, dtype, P=P, transport=transport) as fs:
        run_operator(fs, d0, u, v, w, want, f"N={N} P={P} {transport} {advect_form}")
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


# ---- §9: the three-field kernels inside vel_step, long traces ----------------------------------------------------
_STEPS = Cache()
STEP_K, STEP_FORCES = 2, dict(eps=0.3, beta=-1.5, ambient=0.0, axis=2)


def step_state(N, dtype):
    f = {n: C.normal_field(N, dtype, 500 + N + q, 0.02) for q, n in enumerate(NAMES)}
    f["u"], f["v"], f["w"] = C.mixed_flow(N, dtype, N)
    return f


def advecting_cfl(f, K):
    """max |dt0 u| over the three components of the velocity vel_step advects with: the state after add_source,
    diffuse and the first projection (SPEC §3), computed with the oracle's operators."""
    T = f["u"].dtype.type
    g = {n: f[n].copy() for n in ("u", "v", "w", "u0", "v0", "w0")}
    for x in "uvw":
        O.add_source(g[x], g[x + "0"], T(DT))
    for b, x in ((1, "u"), (2, "v"), (3, "w")):
        O.diffuse(b, g[x + "0"], g[x], T(VISC), T(DT), K)
    O.project(g["u0"], g["v0"], g["w0"], g["u"], g["v"], K)
    N = f["u"].shape[0] - 2
    return max(float(np.abs(T(DT) * T(N) * g[x + "0"][1:-1, 1:-1, 1:-1]).max()) for x in "uvw")


def step_reference(N, dtype, forces):
    def build():
        f = step_state(N, dtype)
        cfl = advecting_cfl(f, STEP_K)
        want = {n: a.copy() for n, a in f.items()}
        after = []
        for _ in range(2):
            M.step(want, DT, DIFF, VISC, STEP_K, velocity=MC, density=SL, **(STEP_FORCES if forces else {}))
            after.append({n: a.copy() for n, a in want.items()})
        return f, cfl, after

    return _STEPS.get((N, C.dname(dtype), forces), build)


STEP_CASES = [(N, t, forces, form) for N in (13, 34, 65, 70, 130) for t in C.DTYPES for forces in (False, True)
              for form in FORMS]


@pytest.mark.parametrize("N,dtype,forces,advect_form", STEP_CASES, indirect=["advect_form"],
                         ids=[f"N{N}-{C.dname(t)}-{'forces' if g else 'plain'}-{f}" for N, t, g, f in STEP_CASES])
def test_vel_step_maccormack_long_traces(N, dtype, forces, advect_form):
    """Two steps, velocity scheme MacCormack, from mixed_flow: advect_mc_row_kernel<T, 3, *> (the gather form for
    SF_ADVECT_ROW=0) with traces of more than a cell, rows across wave seams, ragged last waves. Once plain, once with
    both forces of §8 on."""
    f, cfl, after = step_reference(N, dtype, forces)
    print(f"N={N} {C.dname(dtype)}: max |dt0 u| of the advecting velocity {cfl:.3f}")
    assert cfl > 1.5, "the velocity left by the first projection no longer traces over cells"
    with make(N, dtype, K=STEP_K) as fs:
        for n, a in f.items():
            fs.upload(n, a)
        fs.set_advection(MC, SL)
        if forces:
            fs.set_vorticity_confinement(STEP_FORCES["eps"])
            fs.set_buoyancy(STEP_FORCES["beta"], STEP_FORCES["ambient"], STEP_FORCES["axis"])
        for s in range(2):
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            for n in NAMES:
                assert_same_bits(fs.download(n), after[s][n], f"N={N} {advect_form} step {s}: {n}")


# ---- §9: special values ------------------------------------------------------------------------------------------
_SPECIAL = Cache()


def special_reference(N, dtype):
    def build():
        u, v, w = C.mixed_flow(N, dtype, N)
        plain = C.normal_field(N, dtype, N)
        d0 = C.special_values(plain, np.random.RandomState(N))
        rng = np.random.RandomState(N + 1)
        su, sv, sw = (C.special_values(c, rng) for c in (u, v, w))
        z = np.zeros_like(d0)
        fields = [M.advect_mc(b, z.copy(), d0, u, v, w, DT) for b in (0, 1)] + [None, None]
        vels = [M.advect_mc(0, z.copy(), plain, su, sv, sw, DT), None, None, M.advect_mc(3, z.copy(), plain, su, sv, sw, DT)]
        return (d0, u, v, w, fields), (plain, su, sv, sw, vels)

    return _SPECIAL.get((N, C.dname(dtype)), build)


SPECIAL_CASES = [(N, t, form) for N in (34, 70) for t in C.DTYPES for form in FORMS]


@pytest.mark.parametrize("N,dtype,advect_form", SPECIAL_CASES, indirect=["advect_form"],
                         ids=[f"N{N}-{C.dname(t)}-{f}" for N, t, f in SPECIAL_CASES])
def test_maccormack_special_values(N, dtype, advect_form):
    """d0 with NaN, infinities, zeros of both signs and ties under a clean velocity (the select forms of mn / mx and the
    limiter's comparisons decide bits here), then a clean d0 under a velocity with a few NaN / infinite cells (SPEC §3:
    a NaN position reads index 0, an infinite one a wall; legal inputs)."""
    in_field, in_velocity = special_reference(N, dtype)
    with make(N, dtype) as fs:
        run_operator(fs, *in_field, f"N={N} {advect_form} special d0", nan_ok=True)
        run_operator(fs, *in_velocity, f"N={N} {advect_form} special velocity", nan_ok=True)


# ---- §8 ----------------------------------------------------------------------------------------------------------
FORCE_MODES = {"vort": dict(eps=0.35), "buoy": dict(beta=1.7, ambient=0.1, axis=0),
               "both": dict(eps=0.35, beta=1.7, ambient=0.1, axis=2)}


def run_force_operators(fs, f, what, nan_ok=False, modes=FORCE_MODES):
    N = f["u"].shape[0] - 2
    for n, a in f.items():
        fs.upload(n, a)
    fs.upload("user0", np.full((N + 2,) * 3, 7.0, f["u"].dtype))
    fs.vorticity_magnitude("u", "v", "w", "user0")
    fs.sync()
    assert_same_bits(fs.download("user0"), F.vorticity(f["u"], f["v"], f["w"]), f"{what}: |omega|", nan_ok)
    for mode, coef in modes.items():
        want = {n: a.copy() for n, a in f.items()}
        with np.errstate(all="ignore"):
            F.add_forces(want["u"], want["v"], want["w"], want["dens"], want["u0"], want["v0"], want["w0"], **coef)
        for n in ("u0", "v0", "w0"):
            fs.upload(n, f[n])
        set_forces(fs, **coef)
        fs.add_forces("u", "v", "w", "dens", "u0", "v0", "w0")
        fs.sync()
        for n in NAMES:
            assert_same_bits(fs.download(n), want[n], f"{what} {mode}: {n}", nan_ok)


@pytest.mark.parametrize("N,dtype", C.SHAPES, ids=[f"N{N}-{C.dname(t)}" for N, t in C.SHAPES])
def test_forces(N, dtype):
    """sf_vorticity_magnitude and sf_add_forces (vorticity, buoyancy, both) on fields with a block of uniform |omega|
    (len = 0), sources updated in place; then a step with both forces and bound sources (the sources read from the bound
    slots, their shells copied)."""
    f = C.forces_fields(N, dtype, 11 + N)
    K = 2
    with make(N, dtype, K=K) as fs:
        run_force_operators(fs, f, f"N={N}")
    src = {n: C.normal_field(N, dtype, 40 + N + q, 0.2) for q, n in enumerate(USER)}
    for mode in ("both",) if N > 70 else tuple(FORCE_MODES):
        want = {n: a.copy() for n, a in f.items()}
        F.step(want, DT, DIFF, VISC, K, bound=src, **FORCE_MODES[mode])
        with make(N, dtype, K=K) as fs:
            for n, a in f.items():
                fs.upload(n, a)
            for n, slot in USER.items():
                fs.upload(slot, src[n])
            fs.bind_sources()
            set_forces(fs, **FORCE_MODES[mode])
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            for n in NAMES:
                assert_same_bits(fs.download(n), want[n], f"N={N} bound {mode}: {n}")
            for n, slot in USER.items():
                assert_same_bits(fs.download(slot), src[n], f"N={N} bound {mode}: slot {slot}")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,P,transport", C.DECOMPOSED, ids=[f"N{n}-P{p}-{t}" for n, p, t in C.DECOMPOSED])
def test_forces_on_slabs(N, P, transport, dtype):
    f = C.forces_fields(N, dtype, 11 + N)
    with make(N, dtype, P=P, transport=transport) as fs:
        run_force_operators(fs, f, f"N={N} P={P} {transport}")


@pytest.mark.parametrize("N,dtype", C.SHAPES, ids=[f"N{N}-{C.dname(t)}" for N, t in C.SHAPES])
def test_zero_coefficients_evaluate_nothing(N, dtype):
    """SPEC §8: a term whose coefficient is zero is not evaluated. eps = 0 with -0 sources and NaN in the velocity,
    beta = 0 with NaN in dens: what the term would have touched comes back bit for bit."""
    f = C.zero_coefficient_inputs(N, dtype)
    modes = {"eps=0": dict(eps=0.0, beta=1.7, ambient=0.1, axis=1), "beta=0": dict(eps=0.35, beta=0.0, axis=1),
             "both zero": dict(eps=0.0, beta=0.0, axis=1)}
    with make(N, dtype) as fs:
        run_force_operators(fs, f, f"N={N}", nan_ok=True, modes=modes)
        for n in ("u0", "v0", "w0"):
            fs.upload(n, f[n])
        set_forces(fs, **modes["eps=0"])
        fs.add_forces("u", "v", "w", "dens", "u0", "v0", "w0")
        fs.sync()
        for n in ("u0", "w0"):  # the NaN velocity reached nothing, the -0 sources kept their sign
            assert_same_bits(fs.download(n), f[n], f"N={N} eps=0: {n}")
        assert np.isnan(fs.download("v0")).sum() == 1  # dens[1, N, 1] through the buoyancy, nothing else


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_force_closed_forms_on_the_smallest_grids(N, dtype):
    """SPEC §8.1 through the C ABI where every interior cell is an edge and a corner: the rigid rotation (uniform
    |omega| = 2N, f = 0 bitwise) and the shear v = i^2 (|omega| = 2 N i; fx = fz = 0 and fy within 8 eps of -2 eps i for
    N >= 2; at N = 1 the mirrored shells make |omega| uniform and f = 0 exactly)."""
    eps = 0.3
    k, j, i = np.meshgrid(*(np.arange(N + 2, dtype=np.float64),) * 3, indexing="ij")
    zero = np.zeros((N + 2,) * 3, dtype)
    c = N // 2
    profiles = {"shear": (zero, (i * i).astype(dtype), zero),
                "rotation": ((c - j).astype(dtype), (i - c).astype(dtype), zero)}
    inner = (slice(1, -1),) * 3
    with make(N, dtype) as fs:
        fs.set_vorticity_confinement(eps)
        for name, (u, v, w) in profiles.items():
            for n, a in (("u", u), ("v", v), ("w", w), ("dens", zero), ("u0", zero), ("v0", zero), ("w0", zero)):
                fs.upload(n, a)
            fs.vorticity_magnitude("u", "v", "w", "user0")
            fs.add_forces("u", "v", "w", "dens", "u0", "v0", "w0")
            fs.sync()
            mag = fs.download("user0")
            got = [fs.download(n) for n in ("u0", "v0", "w0")]
            assert_same_bits(mag, F.vorticity(u, v, w), f"{name}: |omega|")
            ref = [zero.copy(), zero.copy(), zero.copy()]
            F.add_forces(u, v, w, zero, *ref, eps=eps)
            for a, r, n in zip(got, ref, "uvw"):
                assert_same_bits(a, r, f"{name}: source of {n}")
            if name == "rotation":
                assert (mag[inner] == 2 * N).all()
                assert not any(a.any() for a in got)
            elif N == 1:
                assert (mag == mag[1, 1, 1]).all()
                assert not any(a.any() for a in got)
            else:
                assert np.array_equal(mag[inner], np.broadcast_to(2 * N * np.arange(1, N + 1), (N, N, N)))
                assert not got[0].any() and not got[2].any()
                want = -2.0 * eps * np.arange(1, N + 1)
                assert np.all(np.abs(got[1][inner].astype(np.float64) - want) <= 8 * np.finfo(dtype).eps * np.abs(want))


# ---- §10 ---------------------------------------------------------------------------------------------------------
def reduction_inputs(N, dtype):
    """(x, state), plain and through special_values: magnitudes over five decades; the state's velocities scaled to a
    CFL of a few cells."""
    x = C.decades_field(N, dtype, 300 + N)
    f = {n: (C.decades_field(N, dtype, 400 + N + q).astype(np.float64) / (10.0 * DT * N)).astype(dtype)
         for q, n in enumerate(("u", "v", "w"))}
    f["dens"] = C.decades_field(N, dtype, 404 + N)
    rng = np.random.RandomState(600 + N)
    return (x, f), (C.special_values(x, rng), {n: C.special_values(a, rng) for n, a in f.items()})


def run_reductions(fs, N, dtype, what):
    for kind, (x, f) in zip(("plain", "special"), reduction_inputs(N, dtype)):
        fs.upload("user1", x)
        for n in STATE:
            fs.upload(n, f[n])
        check_reduce(fs, "user1", x, f"{what} {kind}")
        check_diag(fs, f, f"{what} {kind}")
        assert_same_bits(fs.download("user1"), x, f"{what} {kind}: user1 after the calls", nan_ok=True)
        for n in STATE:
            assert_same_bits(fs.download(n), f[n], f"{what} {kind}: {n} after the calls", nan_ok=True)


@pytest.mark.parametrize("N,dtype", C.REDUCE_SHAPES, ids=[f"N{N}-{C.dname(t)}" for N, t in C.REDUCE_SHAPES])
def test_reductions_and_diagnostics(N, dtype):
    """Every op and the diagnostics struct at P = 1. N = 130, 200 (fp64) and 260, 324 (fp32) take the second trip of the
    row partial (m >= 1); 65 and 130 pad half of the plane fold."""
    with make(N, dtype) as fs:
        run_reductions(fs, N, dtype, f"N={N}")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,P,transport", C.DECOMPOSED, ids=[f"N{n}-P{p}-{t}" for n, p, t in C.DECOMPOSED])
def test_reductions_on_slabs_equal_one_slab(N, P, transport, dtype):
    """The reference does not depend on P: P slabs give the bits of P = 1 (test_reductions_and_diagnostics)."""
    with make(N, dtype, P=P, transport=transport) as fs:
        run_reductions(fs, N, dtype, f"N={N} P={P} {transport}")
