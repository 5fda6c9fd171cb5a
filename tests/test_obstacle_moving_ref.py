"""The numpy reference of docs/SPEC.md §19 (tests/obstacle_moving_ref.py) on the CPU: what it owes to §15 / §17, its
closed forms, and that the inputs of tests/obstacle_moving_cases.py, which tests/test_obstacle_moving_gpu.py runs on
the device, tell each wrong reading of §19 from the right one. No GPU and no library."""
import numpy as np
import pytest

import obstacle_cases as OC
import obstacle_moving_cases as MV
import obstacle_moving_ref as MR
import obstacle_transport_cases as TC
import obstacle_transport_ref as TR
import obstacles_mg_ref as OM
import obstacles_ref as OB
import shape_cases as C
import stable_ref as S3
from gpu_support import DT, assert_same_bits

I3 = MR.I3
DTYPES = C.DTYPES
IDS = [C.dname(t) for t in DTYPES]


def same(got, want, what):
    assert_same_bits(got, want, what)


def differs(a, b):
    uint = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool((a.view(uint) != b.view(uint)).any())


def project(family, N, dtype, vs, m=0, mg=None, wrong=None, slabs=1, mask=None):
    mask = OC.mask(family, N, dtype) if mask is None else mask
    return MR.project_cg(*MV.project_fields(family, N, dtype), mask, vs, MV.TOL, MV.ITERS, m, mg, slabs, wrong)


def diffused(family, N, dtype, b, K, vs, wrong=None, mask=None, slabs=1):
    x, x0 = TC.fields(family, N, dtype, b)
    MR.diffuse(b, x, x0, MV.DIFF, DT, K, OC.mask(family, N, dtype) if mask is None else mask, vs, wrong, slabs)
    return x


def advected(family, N, dtype, b, vs, wrong=None, mask=None, slabs=1, one_plane=False):
    d0 = TC.fields(family, N, dtype, b)[1]
    d = np.zeros_like(d0)
    MR.advect(b, d, d0, *TC.velocity(family, N, dtype, one_plane), DT, OC.mask(family, N, dtype) if mask is None else mask,
              vs, wrong, slabs)
    return d


def transport_vs(family, N, dtype):
    return MV.solid_velocity(family, N, dtype, MV.transport_scale(N))


# ---- the conditions of the cases the GPU file runs --------------------------------------------------------------------
@pytest.mark.parametrize("family", MV.FAMILIES)
@pytest.mark.parametrize("N", [13, 34])
def test_conditions_hold(family, N):
    dtype = np.float32
    mask = OC.mask(family, N, dtype)
    vs = MV.solid_velocity(family, N, dtype)
    out = project(family, N, dtype, vs)
    nans = sum(int(np.isnan(out[n]).sum()) for n in ("u", "v", "w", "p", "div"))
    for b in MV.BS:
        nans += int(np.isnan(diffused(family, N, dtype, b, 2, transport_vs(family, N, dtype))).sum())
        nans += int(np.isnan(advected(family, N, dtype, b, transport_vs(family, N, dtype))).sum())
    assert nans == 0
    share, closed = MV.fluid_share(mask), MV.closed_face_cells(mask)
    hits, _ = MV.advect_facts(mask, TC.velocity(family, N, dtype))
    print(f"{family} N={N}: fluid share {share:.3f}, fluid cells with a closed face on i, j, k {closed}, "
          f"fluid cells with a solid sample {hits}")
    if family in MV.DEGENERATE:
        return
    assert share >= 0.25
    assert hits >= 100
    if (family, N) == ("box", 13):
        # The one case that cannot reach 100: the centred box of obstacle_cases is 4^3 cells at N = 13, so exactly
        # 2 * 4^2 = 32 fluid cells touch it on each axis. Held to that count; box reaches 200 per axis at N = 34, and
        # the other three families pass 100 at N = 13 (docs/SPEC.md §19.1).
        assert closed == (32, 32, 32)
    else:
        assert min(closed) >= 100


def test_conditions_of_the_row_masks():
    for N, dtype in MV.ROW_SHAPES[:1] + MV.ROW_SHAPES[2:3]:
        mask = MV.row_mask(N, dtype)
        mk = OB.Mask(mask)
        W = 16 // np.dtype(dtype).itemsize
        for idx in (64 * W - 1, 64 * W, N - 1):
            col_solid, col_closed = mk.solid[:, :, idx], (mk.closed["ilo"] | mk.closed["ihi"])[:, :, idx] & mk.fluid[:, :, idx]
            assert col_solid.sum() >= 100 and col_closed.sum() >= 100, (N, idx)
        assert MV.fluid_share(mask) >= 0.25


# ---- zero velocity: §15 / §17 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [13, 34])
def test_zero_velocity_gives_the_bits_of_15_and_17(N, dtype):
    zero = MV.zero_velocity(N, dtype)
    for family in ("box", "random30"):
        mask = OC.mask(family, N, dtype)
        u, v, w = MV.project_fields(family, N, dtype)
        for m in (0, 2):
            got, want = project(family, N, dtype, zero, m), OB.project_cg(u, v, w, mask, MV.TOL, MV.ITERS, m)
            for n in ("u", "v", "w", "p", "div"):
                same(got[n], want[n], f"{family} m={m}: {n}")
            assert (got["status"], got["iterations"], got["rel_residual"]) == (want["status"], want["iterations"], want["rel_residual"])
        if N == 34 and family == "box":
            got, want = project(family, N, dtype, zero, mg=(2, 0, 8)), OM.project_cg(u, v, w, mask, MV.TOL, MV.ITERS, 2, 0, 8)
            for n in ("u", "v", "w", "p", "div"):
                same(got[n], want[n], f"mg: {n}")
        for b in MV.BS:
            x, x0 = TC.fields(family, N, dtype, b)
            TR.diffuse_masked(b, x, x0, MV.DIFF, DT, 2, mask)
            same(diffused(family, N, dtype, b, 2, zero), x, f"{family} diffuse b={b}")
            d0 = TC.fields(family, N, dtype, b)[1]
            d = np.zeros_like(d0)
            TR.advect_masked(b, d, d0, *TC.velocity(family, N, dtype), DT, mask)
            same(advected(family, N, dtype, b, zero), d, f"{family} advect b={b}")


def test_zero_velocity_turns_a_negative_zero_into_a_positive_one():
    """(0 + 0) - x is +0 where -x is -0: equal, not the same bits, where a fluid cell next to a closed face holds a zero
    on that face's axis."""
    N, dtype = 5, np.float32
    mask = OC.mask("box", N, dtype)
    x = np.zeros((N + 2,) * 3, dtype)
    mk = MR.Moving(mask, MV.zero_velocity(N, dtype))
    faces = 0
    for face in ("ilo", "ihi", "jlo", "jhi", "klo", "khi"):
        e15, e19 = mk.eff(x, face, -1), mk.effv(x, face)
        closed = mk.closed[face]
        assert np.array_equal(e15, e19)
        # the operand across a closed face is -0 under §15 and +0 under §19; across an open one both are the +0 stored
        assert np.signbit(e15[closed]).all() and not np.signbit(e19).any() and not np.signbit(e15[~closed]).any()
        faces += int(closed.sum())
    assert faces > 0
    # a result compares equal all the same
    got = MR.divergence(x, x, x, mk)[1]
    want = OB.divergence(x, x, x, OB.Mask(mask))[1]
    assert np.array_equal(got, want)


# ---- uniform motion -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_uniform_motion(dtype):
    """u = a in all cells and us = a: a fluid cell away from the domain walls sees no obstacle at all."""
    N, a = 13, dtype(0.375)
    mask = OC.mask("box", N, dtype)
    mk = OB.Mask(mask)
    inner = np.zeros((N,) * 3, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    cells = mk.fluid & inner
    assert cells.sum() > 500
    u = np.full((N + 2,) * 3, a, dtype)
    zero = np.zeros_like(u)
    vs = [u.copy(), zero.copy(), zero.copy()]
    div = MR.divergence(u, zero, zero, MR.Moving(mask, vs))[1][I3]
    # every difference is exactly +0, so div is c_div * +0: a zero, of c_div's sign (c_div < 0: -0), as in a free cell
    c_div = dtype(-0.5) * (dtype(1) / dtype(N))
    same(div[cells], np.full(int(cells.sum()), c_div * dtype(0), dtype), "div")
    rng = np.random.RandomState(5)
    x0 = rng.standard_normal(u.shape).astype(dtype)
    got = MR.sweep(1, u, x0, dtype(0.1), dtype(1) / dtype(1.6), MR.Moving(mask, vs))
    cur = u  # an interior cell of the unmasked sweep: its six stored neighbours
    want = np.zeros_like(u)
    want[I3] = (x0[I3] + dtype(0.1) * (((cur[1:-1, 1:-1, :-2] + cur[1:-1, 1:-1, 2:]) + (cur[1:-1, :-2, 1:-1] + cur[1:-1, 2:, 1:-1]))
                                         + (cur[:-2, 1:-1, 1:-1] + cur[2:, 1:-1, 1:-1]))) * (dtype(1) / dtype(1.6))
    same(got[cells], want[I3][cells], "sweep")
    vel = [np.full(u.shape, dtype(0.3 / (DT * N)), dtype), np.full(u.shape, dtype(-0.2 / (DT * N)), dtype),
           np.full(u.shape, dtype(0.45 / (DT * N)), dtype)]
    d, dfree = np.zeros_like(u), np.zeros_like(u)
    MR.advect(1, d, u, *vel, DT, mask, vs)
    S3.advect(1, dfree, u, *vel, DT)
    same(d[I3][cells], dfree[I3][cells], "advect")


# ---- one fluid cell between moving solids ------------------------------------------------------------------------------
def test_one_fluid_cell_between_moving_solids():
    N, dtype = 4, np.float64
    mask = np.ones((N + 2,) * 3, dtype)
    c = (2, 3, 2)  # [k, j, i]: an inner cell
    mask[c] = 0
    u, v, w = (np.zeros(mask.shape, dtype) for _ in range(3))
    us, vs, ws = (np.zeros(mask.shape, dtype) for _ in range(3))
    u[c], v[c], w[c] = 0.5, -0.25, 2.0
    us[2, 3, 1], us[2, 3, 3] = 1.0, 4.0      # low, high along i
    vs[2, 2, 2], vs[2, 4, 2] = -2.0, 0.5     # along j
    ws[1, 3, 2], ws[3, 3, 2] = 8.0, -1.0     # along k
    div = MR.divergence(u, v, w, MR.Moving(mask, [us, vs, ws]))[1]
    c_div = -0.5 * 0.25
    want = c_div * ((((2 * 4.0 - 0.5) - (2 * 1.0 - 0.5)) + ((2 * 0.5 + 0.25) - (2 * -2.0 + 0.25))) + ((2 * -1.0 - 2.0) - (2 * 8.0 - 2.0)))
    assert want == c_div * ((6.0 + 5.0) - 18.0)
    assert div[c] == want
    assert not np.delete(div[I3].ravel(), np.ravel_multi_index((1, 2, 1), (N,) * 3)).any()


# ---- parked NaN, slabs, b = 0 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", MV.MIXED)
def test_parked_nan_gives_the_bits_of_the_clean_input(family):
    N, dtype = 13, np.float32
    mask = OC.mask(family, N, dtype)
    vs, tv = MV.solid_velocity(family, N, dtype), transport_vs(family, N, dtype)
    clean, park = project(family, N, dtype, vs, 2), project(family, N, dtype, MV.parked(vs, mask), 2)
    for n in ("u", "v", "w", "p", "div"):
        same(park[n], clean[n], n)
    for b in MV.BS:
        same(diffused(family, N, dtype, b, 2, MV.parked(tv, mask)), diffused(family, N, dtype, b, 2, tv), f"diffuse {b}")
        same(advected(family, N, dtype, b, MV.parked(tv, mask)), advected(family, N, dtype, b, tv), f"advect {b}")


@pytest.mark.parametrize("slabs", [2, 17])
def test_emulated_slabs_give_the_bits_of_one(slabs):
    N, dtype = 34, np.float32
    mask = OC.mask("walls", N, dtype, slabs)
    vs = MV.solid_velocity("walls", N, dtype)
    one, many = project("walls", N, dtype, vs, 2, mask=mask), project("walls", N, dtype, vs, 2, mask=mask, slabs=slabs)
    for n in ("u", "v", "w", "p", "div"):
        same(many[n], one[n], n)
    assert (many["status"], many["iterations"], many["rel_residual"]) == (one["status"], one["iterations"], one["rel_residual"])


def test_b0_fields_are_those_of_17_with_any_velocity():
    N, dtype = 13, np.float64
    for family in MV.MIXED:
        mask = OC.mask(family, N, dtype)
        x, x0 = TC.fields(family, N, dtype, 0)
        TR.diffuse_masked(0, x, x0, MV.DIFF, DT, 5, mask)
        same(diffused(family, N, dtype, 0, 5, transport_vs(family, N, dtype)), x, "diffuse")
        d = np.zeros_like(x0)
        TR.advect_masked(0, d, x0, *TC.velocity(family, N, dtype), DT, mask)
        same(advected(family, N, dtype, 0, transport_vs(family, N, dtype)), d, "advect")


# ---- the wrong readings ---------------------------------------------------------------------------------------------
# reading -> the operators whose result it changes, on box at N = 13 in fp32 unless a case is named
PROJECT_WRONG = ("no_doubling", "plus_x", "xs_at_c", "wrong_axis", "nb_swapped", "solids_zero_after_project")
SWEEP_WRONG = ("no_doubling", "plus_x", "xs_at_c", "wrong_axis", "nb_swapped", "no_slip", "solids_set_by_sweep")
ADVECT_WRONG = ("wrong_axis", "wv_at_c", "velocity_of_i0", "solids_set_by_advect")


@pytest.mark.parametrize("family", ["box", "random30"])
def test_wrong_readings_change_the_result(family):
    N, dtype = 13, np.float32
    vs, tv = MV.solid_velocity(family, N, dtype), transport_vs(family, N, dtype)
    right = project(family, N, dtype, vs)
    for wrong in PROJECT_WRONG:
        out = project(family, N, dtype, vs, wrong=wrong)
        assert any(differs(out[n], right[n]) for n in ("u", "v", "w", "div")), wrong
    for b in (1, 2, 3):
        right_sweep, right_advect = diffused(family, N, dtype, b, 1, tv), advected(family, N, dtype, b, tv)
        for wrong in SWEEP_WRONG:
            assert differs(diffused(family, N, dtype, b, 1, tv, wrong), right_sweep), (wrong, b)
        for wrong in ADVECT_WRONG:
            assert differs(advected(family, N, dtype, b, tv, wrong), right_advect), (wrong, b)
    assert differs(diffused(family, N, dtype, 0, 1, tv, "effv_b0"), diffused(family, N, dtype, 0, 1, tv)), "effv_b0"


def test_a_fluid_entry_as_an_operand_shows_as_nan_when_parked():
    N, dtype, family = 13, np.float32, "box"
    mask = OC.mask(family, N, dtype)
    vs, tv = MV.parked(MV.solid_velocity(family, N, dtype), mask), MV.parked(transport_vs(family, N, dtype), mask)
    assert np.isnan(project(family, N, dtype, vs, wrong="fluid_entry")["div"]).any()
    assert np.isnan(diffused(family, N, dtype, 1, 1, tv, "fluid_entry")).any()
    assert np.isnan(advected(family, N, dtype, 1, tv, "fluid_entry")).any()
    assert np.isnan(project(family, N, dtype, vs, wrong="xs_at_c")["div"]).any()
    assert np.isnan(advected(family, N, dtype, 2, tv, "wv_at_c")).any()


def test_a_stale_ghost_plane_of_the_solid_velocity_shows_under_walls():
    N, dtype, P = 34, np.float32, 2
    mask = OC.mask("walls", N, dtype, P)
    vs, tv = MV.solid_velocity("walls", N, dtype), transport_vs("walls", N, dtype)
    right = project("walls", N, dtype, vs, mask=mask)
    assert differs(project("walls", N, dtype, vs, mask=mask, wrong="xs_ghost_stale", slabs=P)["div"], right["div"])
    assert differs(diffused("walls", N, dtype, 3, 1, tv, "xs_ghost_stale", mask, P), diffused("walls", N, dtype, 3, 1, tv, mask=mask))
    for b in (1, 2, 3):
        assert differs(advected("walls", N, dtype, b, tv, "xs_ghost_stale", mask, P, True),
                       advected("walls", N, dtype, b, tv, mask=mask, one_plane=True)), b


# ---- a moved box ----------------------------------------------------------------------------------------------------
def test_a_moved_box():
    N = MV.MOVED_N
    (m0, vs, vel0, dens0), (m1, _, vel1, dens1) = MV.moved_box_sequence()
    s0, s1 = OB.Mask(m0).solid, OB.Mask(m1).solid
    uncovered = s0 & ~s1
    assert uncovered.sum() == (OC.box_range(N)[1] - OC.box_range(N)[0] + 1) ** 2
    # the cells the box uncovers enter the second step with the solid's velocity and no density
    same(vel0["u"][I3][uncovered], vs[0][I3][uncovered], "u of the uncovered cells")
    assert not vel0["v"][I3][uncovered].any() and not vel0["w"][I3][uncovered].any()
    assert not dens0[I3][uncovered].any() and not np.signbit(dens0[I3][uncovered]).any()
    # after the second step the solid cells hold the solid's velocity, and the density none
    same(vel1["u"][I3][s1], vs[0][I3][s1], "u of the solid cells")
    assert not dens1[I3][s1].any()
    assert not any(np.isnan(x).any() for x in (vel1["u"], vel1["v"], vel1["w"], dens1))
