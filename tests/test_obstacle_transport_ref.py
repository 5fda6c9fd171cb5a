"""CPU tests of tests/obstacle_transport_ref.py, the numpy reference of docs/SPEC.md §17 (mask-aware transport): what
the SPEC promises of the masked diffusion and advection holds on the reference itself, and every wrong reading of §17
that the reference can be switched to (obstacle_transport_ref.WRONG) changes the result of a named case of
tests/obstacle_transport_cases.py, so the GPU tests against this reference tell each of them from the SPEC's reading."""
import numpy as np
import pytest

import obstacle_cases as OC
import obstacle_transport_cases as TC
import obstacle_transport_ref as TR
import obstacles_ref as OB
import shape_cases as C
import stable_ref as S3
from ref_support import same_bits

I = TR.I
DTYPE_IDS = ["f32", "f64"]


def advected(family, N, dtype, b, wrong=None, d0=None, slabs=1, one_plane=False, mask=None):
    mask = OC.mask(family, N, dtype) if mask is None else mask
    d0 = TC.fields(family, N, dtype, b)[1] if d0 is None else d0
    d = np.zeros_like(d0)
    TR.advect_masked(b, d, d0, *TC.velocity(family, N, dtype, one_plane), TC.DT, mask, wrong, slabs)
    return d


def swept(family, N, dtype, b, K, wrong=None, x=None, x0=None):
    fx, fx0 = TC.fields(family, N, dtype, b)
    out = (fx if x is None else x).copy()
    TR.lin_solve_masked(b, out, fx0 if x0 is None else x0, TC.A, 1 + 6 * TC.A, K, OC.mask(family, N, dtype), wrong)
    return out


# ---- an empty mask gives the bits of §3 -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", [13, 34])
@pytest.mark.parametrize("b", TC.BS)
def test_empty_mask_is_section_3(N, dtype, b):
    x, x0 = TC.fields("empty", N, dtype, b)
    want = x.copy()
    S3.lin_solve(b, want, x0, TC.A, 1 + 6 * TC.A, 5)
    assert same_bits(swept("empty", N, dtype, b, 5), want)
    want = np.zeros_like(x0)
    S3.advect(b, want, x0, *TC.velocity("empty", N, dtype), TC.DT)
    assert same_bits(advected("empty", N, dtype, b), want)


def test_no_sweep_is_a_no_op():
    x, _ = TC.fields("box", 13, np.float32)
    assert same_bits(swept("box", 13, np.float32, 0, 0), x)


# ---- conservation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["box", "random30", "walls"])
@pytest.mark.parametrize("N", [13, 34])
def test_masked_diffusion_conserves_what_zeroing_destroys(family, N):
    """b = 0, fp64, a = 0.1, K = 40, a random density on the fluid cells, its shells mirrored. The masked sweeps keep the
    sum over the fluid cells to rounding (each face's flux enters one cell and leaves the other; a closed face and a
    mirrored wall carry none); §15's diffuse followed by zero_solid loses what leaked into the solids."""
    dtype, K = np.float64, 40
    mask = OC.mask(family, N, dtype)
    mk = OB.Mask(mask)
    x0 = np.zeros((N + 2,) * 3, dtype)
    x0[I] = np.where(mk.fluid, np.random.RandomState(TC.seed(family, N)).random_sample((N,) * 3), 0.0)
    S3.set_bnd(0, x0)
    total = x0[I][mk.fluid].sum()
    x = x0.copy()
    TR.lin_solve_masked(0, x, x0, TC.A, 1 + 6 * TC.A, K, mask)
    masked = abs(x[I][mk.fluid].sum() - total) / total
    y = x0.copy()
    S3.lin_solve(0, y, x0, TC.A, 1 + 6 * TC.A, K)
    OB.zero_solids(y, mask)
    zeroed = abs(y[I][mk.fluid].sum() - total) / total
    print(f"{family} N={N}: relative change of the fluid's sum: masked {masked:.3e}, diffuse + zero_solid {zeroed:.3e}")
    assert masked < 1e-12
    assert zeroed > 1e-3
    assert not x[I][mk.solid].any()


# ---- all solid and one fluid cell ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("b", TC.BS)
def test_all_solid_is_zero(dtype, b):
    N = 13
    for out in (swept("all_solid", N, dtype, b, 2), advected("all_solid", N, dtype, b)):
        assert not out.any()
        assert same_bits(out[I], np.zeros((N,) * 3, dtype))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
def test_one_fluid_cell(dtype):
    """Every face of the cell is closed (or a mirrored wall when it lies on one): for b = 0 every operand is the cell
    itself, x' = (x0 + a 6x) inv when it lies inside; every solid sample of advect carries d0[c]."""
    T = np.dtype(dtype).type
    inside = [N for N in TC.SIZES if N <= 34
              and (lambda c: 0 < c.min() and c.max() < N - 1)(np.argwhere(OB.Mask(OC.mask("one_fluid", N, dtype)).fluid)[0])]
    N = inside[-1]  # (a size whose fluid cell has six solid neighbours and no shell cell among its samples)
    mask = OC.mask("one_fluid", N, dtype)
    mk = OB.Mask(mask)
    (k, j, i), = np.argwhere(mk.fluid)
    x, x0 = TC.fields("one_fluid", N, dtype)
    got = swept("one_fluid", N, dtype, 0, 1)
    a, inv = T(TC.A), T(1) / T(1 + 6 * TC.A)
    c = x[I][k, j, i]
    want = (x0[I][k, j, i] + a * (((c + c) + (c + c)) + (c + c))) * inv
    assert got[I][k, j, i] == want
    assert np.count_nonzero(got[I]) == 1
    # advect: a constant field of samples, whatever the weights: s0 (t0 (r0 c + r1 c) + ...) + s1 (...)
    d0 = x0
    u, v, w = (0.3 / (TC.DT * N) * f for f in TC.velocity("one_fluid", N, dtype))  # (the trace stays next to the cell)
    d = np.zeros_like(d0)
    TR.advect_masked(0, d, d0, u, v, w, TC.DT, mask)
    flat = d0.copy()
    flat[...] = d0[I][k, j, i]
    want = np.zeros_like(d0)
    S3.advect(0, want, flat, u, v, w, TC.DT)
    assert d[I][k, j, i] == want[I][k, j, i] and np.count_nonzero(d[I]) == 1


# ---- parked NaN ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("family", ["box", "random30", "walls", "one_fluid", "special"])
@pytest.mark.parametrize("b", TC.BS)
def test_nan_parked_in_solid_cells_reaches_nothing(family, dtype, b):
    N = 13
    solid = OB.Mask(OC.mask(family, N, dtype)).solid
    x, x0 = TC.fields(family, N, dtype, b)
    px, px0 = OC.parked_nan((x, x0), solid)
    got = swept(family, N, dtype, b, 3, x=px, x0=px0)
    assert np.isfinite(got).all() and same_bits(got, swept(family, N, dtype, b, 3))
    got = advected(family, N, dtype, b, d0=px0)
    assert np.isfinite(got).all() and same_bits(got, advected(family, N, dtype, b))


# ---- wrong readings -----------------------------------------------------------------------------------------------------
# per wrong reading: (operator, family, N, dtype, b) of a case that tells it from §17
SEPARATES = {
    "closed_stored": ("sweep", "box", 13, np.float32, 0),
    "eff_everywhere": ("sweep", "box", 13, np.float64, 1),
    "no_slip": ("sweep", "random30", 13, np.float32, 2),
    "solids_not_zeroed": ("sweep", "box", 13, np.float32, 3),
    "sample_stored": ("advect", "box", 13, np.float32, 0),
    "wv_zero_b0": ("advect", "box", 13, np.float64, 0),
    "wv_own_bn": ("advect", "random30", 13, np.float32, 1),
    "solidity_of_i0": ("advect", "random30", 13, np.float64, 0),
    "shell_solid": ("advect", "walls", 13, np.float32, 0),
    "code_ghost_stale": ("advect2", "walls", 34, np.float32, 0),
    "dens_zero_solid": ("dens_step", "box", 13, np.float32, 0),
}


def test_every_wrong_reading_has_a_case():
    assert set(SEPARATES) == set(TR.WRONG)


@pytest.mark.parametrize("wrong", TR.WRONG)
def test_a_named_case_separates_each_wrong_reading(wrong):
    op, family, N, dtype, b = SEPARATES[wrong]
    mask = OC.mask(family, N, dtype)
    solid = OB.Mask(mask).solid
    if op == "sweep":
        pairs = [(swept(family, N, dtype, b, 2, wrong), swept(family, N, dtype, b, 2))]
    elif op == "advect":
        pairs = [(advected(family, N, dtype, b, wrong), advected(family, N, dtype, b))]
        if wrong == "sample_stored":  # also where the solids hold zeros, and where they hold a NaN
            d0 = TC.fields(family, N, dtype, b)[1]
            zeroed = d0.copy()
            zeroed[I][solid] = 0
            parked = OC.parked_nan((d0,), solid)[0]
            pairs += [(advected(family, N, dtype, b, wrong, d0=z), advected(family, N, dtype, b, d0=z))
                      for z in (zeroed, parked)]
    elif op == "advect2":  # two emulated slabs, solids on both sides of their boundary (seam_planes)
        m2 = OC.mask(family, N, dtype, 2)
        pairs = [(advected(family, N, dtype, b, wrong, slabs=2, one_plane=True, mask=m2),
                  advected(family, N, dtype, b, slabs=2, one_plane=True, mask=m2))]
    else:
        f = TC.fields(family, N, dtype, b)
        vel = [0.5 * x for x in TC.velocity(family, N, dtype)]
        pairs = [(TR.dens_step(f[0], f[1], *vel, mask, 4, TC.DT, TC.DIFF, wrong=wrong),
                  TR.dens_step(f[0], f[1], *vel, mask, 4, TC.DT, TC.DIFF))]
    for n, (got, want) in enumerate(pairs):
        differ = int((got.view(np.uint8) != want.view(np.uint8)).reshape(got.shape + (-1,)).any(-1).sum())
        print(f"{wrong}: {op} {family} N={N} {C.dname(dtype)} b={b} [{n}]: {differ} entries differ")
        assert differ, f"{wrong} leaves the bits of the reference on its case"


# ---- the cases compare numbers --------------------------------------------------------------------------------------------
ADVECT_CASES = ([(f, N, t, False, 1) for f in TC.FAMILIES for N in TC.SIZES for t in C.DTYPES]
                + [(f, N, np.float32 if P != 17 else np.float64, True, P) for N, P in TC.DECOMPOSED
                   for f in ("walls", "random30")])


@pytest.mark.parametrize("family,N,dtype,one_plane,slabs", ADVECT_CASES,
                         ids=[f"{f}-N{n}-{C.dname(t)}-P{p}" for f, n, t, _, p in ADVECT_CASES])
def test_conditions_hold(family, N, dtype, one_plane, slabs):
    """Cap on what a comparison can hide, for every advect case of the GPU file, on the mask and the velocity that case
    uses: fewer than a quarter of each compared field is NaN; at least a quarter of the interior is fluid
    outside the degenerate families; from N = 13 on at least 100 fluid cells of a family with both kinds of cells take
    a solid sample; on one slab at least 20 traces are longer than one cell."""
    mask = OC.mask(family, N, dtype, slabs if slabs > 1 else None)
    mk = OB.Mask(mask)
    if family not in OC.DEGENERATE:
        assert 4 * mk.n_fluid >= N ** 3
    vel = TC.velocity(family, N, dtype, one_plane)
    hits, far = TC.advect_facts(mask, vel, slabs)
    nans = []
    for b in TC.BS:
        for out in (advected(family, N, dtype, b, one_plane=one_plane, mask=mask), swept(family, N, dtype, b, 2)):
            nans.append(int(np.isnan(out).sum()))
            assert 4 * nans[-1] < out.size
    print(f"{family} N={N} {C.dname(dtype)} slabs={slabs}: fluid {mk.n_fluid} of {N ** 3}, {hits} fluid cells with a solid "
          f"sample, {far} traces longer than one cell on one slab, NaN entries at most {max(nans)}")
    if N >= 13:
        assert far >= 20
        if family in TC.MIXED:
            assert hits >= 100
