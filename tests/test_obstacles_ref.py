"""CPU tests of tests/obstacles_ref.py, the numpy reference of docs/SPEC.md §15 (solid obstacles): what the SPEC
promises of the masked projection holds on the reference itself, and every wrong reading of §15 that the reference can
be switched to (obstacles_ref.WRONG) changes the result of a named case of tests/obstacle_cases.py, so the GPU tests
against this reference tell each of them from the SPEC's reading."""
import numpy as np
import pytest

import obstacle_cases as OC
import obstacles_ref as OB
import pressure_cg_ref as R
import pressure_pcg_ref as Q
import shape_cases as C
from ref_support import same_bits

FIELDS = ("u", "v", "w", "p", "div")
DTYPE_IDS = ["f32", "f64"]


def velocity(N, dtype, family="box"):
    return C.cg_velocity(N, dtype, OC.seed(family, N) + 5000)


def same_outcome(a, b):
    return (all(same_bits(a[n], b[n]) for n in FIELDS) and (a["status"], a["iterations"]) == (b["status"], b["iterations"])
            and np.float64(a["rel_residual"]).tobytes() == np.float64(b["rel_residual"]).tobytes())


@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", [13, 34])
@pytest.mark.parametrize("m", [0, 2])
def test_empty_mask_is_the_unmasked_solve(N, dtype, m):
    u, v, w = velocity(N, dtype, "empty")
    mask = OC.mask("empty", N, dtype)
    got = OB.project_cg(u, v, w, mask, OC.TOL, OC.ITERS, m)
    want = Q.project_cg(u, v, w, OC.TOL, OC.ITERS, m)
    assert same_outcome(got, want)
    assert got["iterations"] == OC.ITERS
    assert (np.float64(OB.poisson_residual(got["p"], got["div"], mask)).tobytes()
            == np.float64(R.poisson_residual(want["p"], want["div"])).tobytes())


@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("m", [0, 2])
def test_all_solid_is_a_zero_velocity_at_once(dtype, m):
    N = 13
    u, v, w = velocity(N, dtype, "all_solid")
    out = OB.project_cg(u, v, w, OC.mask("all_solid", N, dtype), OC.TOL, OC.ITERS, m)
    assert (out["status"], out["iterations"], out["rel_residual"]) == (OB.CONVERGED, 0, 0.0)
    for n in ("u", "v", "w", "p", "div"):
        assert not out[n].any(), n  # (zeros everywhere; the shells that mirror with a sign hold -0)
        assert same_bits(out[n][1:-1, 1:-1, 1:-1], np.zeros((N,) * 3, dtype)), n


@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
def test_one_fluid_cell_has_nothing_to_solve(dtype):
    """n_fluid = 1: mu is the cell's divergence, r = 0."""
    N = 13
    out = OB.project_cg(*velocity(N, dtype, "one_fluid"), OC.mask("one_fluid", N, dtype), OC.TOL, OC.ITERS, 2)
    assert (out["status"], out["iterations"], out["rel_residual"]) == (OB.CONVERGED, 0, 0.0)
    assert np.count_nonzero(out["div"][1:-1, 1:-1, 1:-1]) == 1 and not out["p"].any()


@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("family", ["box", "random30", "walls", "one_fluid", "special"])
@pytest.mark.parametrize("m", [0, 2])
def test_nan_parked_in_solid_cells_reaches_nothing(family, dtype, m):
    N = 13
    mask = OC.mask(family, N, dtype)
    solid = OB.Mask(mask).solid
    u, v, w = velocity(N, dtype, family)
    want = OB.project_cg(u, v, w, mask, OC.TOL, OC.ITERS, m)
    got = OB.project_cg(*OC.parked_nan((u, v, w), solid), mask, OC.TOL, OC.ITERS, m)
    for n in FIELDS:
        assert np.isfinite(got[n]).all(), n
    assert same_outcome(got, want)
    # and in p: the residual of the solve is the same with a NaN in every solid cell of the pressure
    p = OC.parked_nan((want["p"],), solid)[0]
    assert OB.poisson_residual(p, want["div"], mask) == OB.poisson_residual(want["p"], want["div"], mask)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("family", ["walls", "random30"])
@pytest.mark.parametrize("slabs", [2, 17])
def test_emulated_slabs_leave_the_bits_of_one(family, dtype, slabs):
    N = 34
    mask = OC.mask(family, N, dtype, slabs)
    u, v, w = velocity(N, dtype, family)
    assert same_outcome(OB.project_cg(u, v, w, mask, OC.TOL, 4, 2, slabs=slabs), OB.project_cg(u, v, w, mask, OC.TOL, 4, 2))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("m", [0, 2, 8])
def test_the_box_converges_as_the_empty_box_does(dtype, m):
    N = OC.CONVERGENCE_N
    # (a random velocity: every mode is in the right-hand side; the smooth field of §11.1 has a handful and converges
    # in the empty box at once, which says nothing about the obstacle)
    u, v, w = C.cg_velocity(N, dtype, C.cg_seed(N))
    box = OB.project_cg(u, v, w, OC.mask("box", N, dtype), OC.TOL, 400, m)
    empty = OB.project_cg(u, v, w, OC.mask("empty", N, dtype), OC.TOL, 400, m)
    print(f"N={N} {C.dname(dtype)} m={m}: box {box['iterations']} iterations (rel {box['rel_residual']:.3e}), "
          f"empty {empty['iterations']} (rel {empty['rel_residual']:.3e})")
    assert box["status"] == empty["status"] == OB.CONVERGED
    assert box["rel_residual"] <= OC.TOL
    # an obstacle must not cost more than half as many iterations again (the box's own count is in §15.1)
    assert box["iterations"] <= 1.5 * empty["iterations"]
    solid = OB.Mask(OC.mask("box", N, dtype)).solid
    for n in ("u", "v", "w"):
        assert not box[n][1:-1, 1:-1, 1:-1][solid].any()


# per wrong reading: (family, N, dtype, m, slabs) of a case that tells it from §15
SEPARATES = {
    "closed_zero": ("box", 13, np.float32, 0, 1),
    "div_stored": ("box", 13, np.float64, 2, 1),
    "mu_n3": ("box", 13, np.float32, 0, 1),
    "grad_unmasked": ("random30", 13, np.float64, 0, 1),
    "solids_not_zeroed": ("box", 13, np.float32, 2, 1),
    "faces_swapped": ("random30", 13, np.float32, 0, 1),
    "nan_solid": ("special", 13, np.float64, 0, 1),
    "ghost_fluid": ("walls", 34, np.float32, 2, 2),
    "r_not_zeroed": ("box", 13, np.float64, 0, 1),
}


def test_every_wrong_reading_has_a_case():
    assert set(SEPARATES) == set(OB.WRONG)


@pytest.mark.parametrize("wrong", OB.WRONG)
def test_a_named_case_separates_each_wrong_reading(wrong):
    family, N, dtype, m, slabs = SEPARATES[wrong]
    mask = OC.mask(family, N, dtype, slabs if slabs > 1 else None)
    u, v, w = velocity(N, dtype, family)
    want = OB.project_cg(u, v, w, mask, OC.TOL, OC.ITERS, m, slabs=slabs)
    got = OB.project_cg(u, v, w, mask, OC.TOL, OC.ITERS, m, slabs=slabs, wrong=wrong)
    differ = [n for n in ("u", "v", "w", "p") if not same_bits(got[n], want[n])]
    print(f"{wrong}: {family} N={N} {C.dname(dtype)} m={m} slabs={slabs}: differs in {differ}")
    assert differ, f"{wrong} leaves the bits of the reference on its case"
    if wrong in ("closed_zero", "faces_swapped", "nan_solid", "ghost_fluid"):  # readings that reach the operator alone
        a = OB.poisson_residual(want["p"], want["div"], mask, slabs)
        b = OB.poisson_residual(want["p"], want["div"], mask, slabs, wrong=wrong)
        assert a != b


@pytest.mark.parametrize("dtype", C.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("family", OC.FAMILIES)
@pytest.mark.parametrize("N", OC.SIZES)
def test_the_cases_compare_numbers_and_keep_fluid(family, N, dtype):
    """Cap on what a comparison can hide: fewer than a quarter of the entries of every compared field are NaN, and at
    least a quarter of the interior is fluid outside the two degenerate families."""
    mask = OC.mask(family, N, dtype)
    mk = OB.Mask(mask)
    assert mk.n_fluid == int((~(mask[1:-1, 1:-1, 1:-1] > 0)).sum())
    if family not in OC.DEGENERATE:
        assert 4 * mk.n_fluid >= N ** 3, (family, N, mk.n_fluid)
    elif family == "all_solid":
        assert mk.n_fluid == 0
    else:
        assert mk.n_fluid == 1
    if N > 34:
        return  # (the solves of the larger sizes are the GPU file's references; the masks are checked above)
    u, v, w = velocity(N, dtype, family)
    for m in (0, OC.SWEEPS):
        out = OB.project_cg(u, v, w, mask, OC.TOL, OC.ITERS, m)
        for n in FIELDS:
            assert 4 * int(np.isnan(out[n]).sum()) < out[n].size, (family, N, m, n)
