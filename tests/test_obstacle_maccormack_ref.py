"""CPU tests of tests/obstacle_maccormack_ref.py, the numpy reference of docs/SPEC.md §18 (MacCormack under the mask):
the facts §18.1 states hold on the reference itself, and every wrong reading of §18 that the reference can be switched
to (obstacle_maccormack_ref.WRONG) changes the result of a named case of tests/obstacle_maccormack_cases.py, so the GPU
tests against this reference tell each of them from the SPEC's reading."""
import numpy as np
import pytest

import maccormack_ref as MR
import obstacle_cases as OC
import obstacle_maccormack_cases as MC
import obstacle_maccormack_ref as MM
import obstacle_transport_ref as TR
import obstacles_ref as OB
import shape_cases as C
from ref_support import same_bits

I = MM.I
F32, F64 = np.float32, np.float64


def differing(got, want):
    return int((got.view(np.uint8) != want.view(np.uint8)).reshape(got.shape + (-1,)).any(-1).sum())


# ---- an empty mask gives the bits of §9 -------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", [(13, F32), (34, F64)], ids=["N13-f32", "N34-f64"])
@pytest.mark.parametrize("b", MC.BS)
def test_empty_mask_is_section_9(N, dtype, b):
    d0, vel = MC.inputs("empty", N, dtype, b)
    want = MR.advect_mc(b, np.zeros_like(d0), d0, *vel, dtype(MC.DT))
    assert differing(MC.want("empty", N, dtype, b), want) == 0


# ---- parked NaN ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["box", "random30", "walls", "special"])
@pytest.mark.parametrize("N", [13, 34, 65])
@pytest.mark.parametrize("b", [0, 2])
def test_nan_parked_in_solid_cells_reaches_nothing(family, N, b):
    dtype = F32
    mask = OC.mask(family, N, dtype)
    d0, vel = MC.inputs(family, N, dtype, b)
    parked = OC.parked_nan((d0,), OB.Mask(mask).solid)[0]
    got = MC.run(mask, parked, vel, b)
    assert np.isfinite(got).all() and same_bits(got, MC.want(family, N, dtype, b))


# ---- fallback cells are first order ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,N", [("box", 13), ("random30", 13), ("walls", 13), ("box", 34)])
def test_fallback_cells_are_advect_masked(family, N):
    dtype, b = F32, 0
    mask = OC.mask(family, N, dtype)
    d0, vel = MC.inputs(family, N, dtype, b)
    p = MM.parts(b, d0, *vel, MC.DT, mask)
    first = np.zeros_like(d0)
    TR.advect_masked(b, first, d0, *vel, MC.DT, mask)
    fb = MM.fallback(p)
    got = MC.want(family, N, dtype, b)
    assert fb.any() and same_bits(got[I][fb], first[I][fb])
    assert same_bits(got[I][p["solid"]], np.zeros(int(p["solid"].sum()), dtype))


# ---- how many cells take each branch ------------------------------------------------------------------------------------
BRANCHES = {("box", 13): dict(fluid=2133, second=1473, limited=48, sf_alone=128, sr_alone=27),
            ("box", 34): dict(fluid=38304, second=33947, limited=1296),
            ("random30", 13): dict(fluid=1523, second=13), ("random30", 34): dict(fluid=27436, second=183),
            ("walls", 13): dict(fluid=1772, second=693), ("walls", 34): dict(fluid=19683, second=3)}


@pytest.mark.parametrize("family,N", list(BRANCHES), ids=[f"{f}-N{n}" for f, n in BRANCHES])
def test_branch_counts(family, N):
    o = MC.second_order_share(family, N, F32)
    print(f"{family} N={N}: {o}")
    for name, n in BRANCHES[family, N].items():
        assert o[name] == n, (name, o)


def test_special_masks_are_nearly_all_fallback():
    for N in (13, 34):
        o = MC.second_order_share("special", N, F32)
        print(f"special N={N}: {o}")
        assert 20 * o["second"] < o["fluid"]


# ---- the cases compare the corrected value and numbers ----------------------------------------------------------------
BOXES = ([("box", N, t, False, None) for N in MC.SIZES if N >= 13 for t in C.DTYPES]
         + [("box", N, MC.decomposed_dtype(P), True, P) for N, P in ((34, 2), (34, 17), (64, 4), (40, 2))])


@pytest.mark.parametrize("family,N,dtype,one_plane,P", BOXES, ids=[f"{f}-N{n}-{C.dname(t)}-P{p}" for f, n, t, _, p in BOXES])
def test_box_cases_are_second_order_on_a_quarter(family, N, dtype, one_plane, P):
    o = MC.check_second_order(family, N, dtype, one_plane, P)
    print(f"{family} N={N} {C.dname(dtype)} P={P}: {o}")
    assert o["second"] > 0


@pytest.mark.parametrize("N", [13, 65, 70])
def test_walls_cases_with_a_corrected_share(N):
    o = MC.second_order_share("walls", N, F32)
    print(f"walls N={N}: {o}")
    assert 10 * o["second"] >= o["fluid"]


# (fp64 up to N = 34: the fp32 case of a size draws the same numbers)
ORDINARY = [(f, N, t) for f, N, t in MC.OPERATORS if t == F32 or N <= 34]


@pytest.mark.parametrize("family,N,dtype", ORDINARY, ids=[f"{f}-N{n}-{C.dname(t)}" for f, n, t in ORDINARY])
def test_nan_share_of_the_ordinary_cases(family, N, dtype):
    mask = OC.mask(family, N, dtype)
    worst = MC.check_nan_share({f"b={b}": MC.want(family, N, dtype, b) for b in MC.BS}, mask, f"{family} N={N}")
    assert worst == 0.0


@pytest.mark.parametrize("N,dtype", MC.SPECIALS, ids=[f"N{n}-{C.dname(t)}" for n, t in MC.SPECIALS])
def test_nan_share_of_the_special_inputs(N, dtype):
    mask = OC.mask("box", N, dtype)
    fields = {f"b={b}": MC.want_special(N, dtype, b) for b in MC.BS}
    worst = MC.check_nan_share(fields, mask, f"specials box N={N}")
    print(f"specials box N={N} {C.dname(dtype)}: worst NaN share {worst:.3f}")
    if N >= 13:
        assert any(np.isnan(x).any() for x in fields.values())  # (the specials reach the compared fields)


# ---- wrong readings -----------------------------------------------------------------------------------------------------
# per wrong reading: (family, N, slabs, inputs) of a case that tells it from §18 (fp32, b = 0), and the entries that
# differ there
SEPARATES = {
    "pass1_unmasked": ("box", 13, 1, "ordinary", 284),
    "no_solid_fallback": ("box", 13, 1, "ordinary", 155),
    "sf_only": ("box", 13, 1, "ordinary", 27),
    "sr_only": ("box", 13, 1, "ordinary", 128),
    "sr_at_forward": ("box", 13, 1, "ordinary", 27),
    "solidity_of_i0_reverse": ("box", 13, 1, "ordinary", 9),
    "solids_not_zeroed": ("random30", 34, 1, "ordinary", 42),
    "hat_ghost_stale": ("box", 34, 2, "one_plane", 506),
    "code_ghost_stale_reverse": ("random30", 34, 2, "one_plane", 17),
    "hw_minmax": ("box", 13, 1, "specials", 51),
}


def test_every_wrong_reading_has_a_case():
    assert set(SEPARATES) == set(MM.WRONG)


@pytest.mark.parametrize("wrong", MM.WRONG)
def test_a_named_case_separates_each_wrong_reading(wrong):
    family, N, slabs, kind, count = SEPARATES[wrong]
    dtype, b = F32, 0
    mask = OC.mask(family, N, dtype, slabs if slabs > 1 else None)
    d0, vel = MC.special_inputs(N, dtype, b) if kind == "specials" else MC.inputs(family, N, dtype, b, kind == "one_plane")
    want = MC.run(mask, d0, vel, b, None, slabs)
    got = MC.run(mask, d0, vel, b, wrong, slabs)
    differ = differing(got, want)
    print(f"{wrong}: {family} N={N} slabs={slabs} {kind}: {differ} entries differ")
    assert differ == count, f"{wrong}: {differ} entries differ on its case, {count} expected"


def test_cases_that_cannot_show_a_reading():
    """What the table's notes say: `box` N = 13 cannot show unzeroed solids, `box` cannot show a stale code plane at
    P = 2."""
    dtype, b = F32, 0
    d0, vel = MC.inputs("box", 13, dtype, b)
    mask = OC.mask("box", 13, dtype)
    assert differing(MC.run(mask, d0, vel, b, "solids_not_zeroed"), MC.run(mask, d0, vel, b)) == 0
    d0, vel = MC.inputs("box", 34, dtype, b, True)
    mask = OC.mask("box", 34, dtype, 2)
    assert differing(MC.run(mask, d0, vel, b, "code_ghost_stale_reverse", 2), MC.run(mask, d0, vel, b, None, 2)) == 0
