"""The numpy reference of docs/SPEC.md §13 (tests/render_view_ref.py) against the closed forms of §13.1, the conditions
the cases of tests/view_cases.py have to meet, and wrong variants of the reference: each is a way a kernel, a carry or a
frame could plausibly go wrong, and each is shown to differ from the reference on a named case — the GPU case of
tests/test_render_view_gpu.py that would catch a library that computed it. No GPU needed."""
import numpy as np
import pytest

import render_cases as RC
import render_ref as RR
import render_view_ref as VR
import view_cases as VC

DTYPE_IDS = ["f32", "f64"]


def same_bits(a, b):
    uint = np.uint32 if a.dtype == np.float32 else np.uint64
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all((a.view(uint) == b.view(uint)) | both_nan))


def same_pair(x, y):
    return same_bits(x[0], y[0]) and same_bits(x[1], y[1])


# ---- (a) the axis identity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", VC.AXIS_SIZES)
def test_axis_frames_equal_the_axis_render(N, dtype):
    dens, emit, sigma = VC.inputs("random", N, dtype)
    for axis, high in RC.VIEWS:
        fr = VR.axis_frame(N, axis, high, sigma)
        for e in (emit, None):
            assert same_pair(VR.render_view(dens, e, fr), RR.render(dens, e, axis, high, sigma)), (N, axis, high)


@pytest.mark.parametrize("dtype", VC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", VC.AXIS_SIZES + [34])
def test_closed_forms(N, dtype):
    """The closed family of §12.1 through the view: exact images on the axis frames, the reference's own §12 render
    there, and (+0, 1) for a zero density along an oblique frame."""
    for axis, high in RC.VIEWS:
        fr = VR.axis_frame(N, axis, high, RC.SIGMA)
        for kind in VC.CLOSED_KINDS:
            dens, emit, sigma = VC.closed(kind, N, dtype, axis, high)
            got = VR.render_view(dens, emit, fr)
            assert same_pair(got, RR.render(dens, emit, axis, high, sigma)), (kind, N, axis, high)
            want = VC.closed_expected(kind, N, dtype, emit, axis, high)
            if want is not None:
                assert same_pair(got, want), (kind, N, axis, high)
            if kind == "half" and VC.half_expected(N, dtype) is not None:
                assert same_pair(VR.render_view(dens, None, fr), VC.half_expected(N, dtype)), (N, axis, high)
    d, step, image = VC.CLOSED_VIEW
    fr = VC.frame(N, d, step, image)
    dens, emit, _ = VC.closed("zero", N, dtype)
    C, Tr = VR.render_view(dens, emit, fr)
    assert same_pair((C, Tr), VR.start(fr, dtype))
    dens, emit, _ = VC.closed("opaque", N, dtype, 2, 0)  # the plane k = 1 opaque: every ray that enters through it ends at Tr = 0
    C, Tr = VR.render_view(dens, emit, fr)
    assert np.count_nonzero(Tr == 0) >= 1 or N < 5


# ---- (b) the chain -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N,P,transport", VC.DECOMPOSED, ids=[f"N{n}-P{p}" for n, p, _ in VC.DECOMPOSED])
def test_the_chain_equals_the_undecomposed_render(N, P, transport, dtype):
    dens, emit, _ = VC.inputs("random", N, dtype)
    for d in range(len(VC.DIRECTIONS)):
        fr = VC.frame(N, d, *VC.CHAIN_VIEW)
        whole = VR.render_view(dens, emit, fr)
        assert same_pair(VR.render_view_slabs(dens, emit, fr, P), whole), (N, P, VC.DIR_IDS[d])
        held = [VR.held_pixels(dens, emit, fr, P, [g]) for g in range(P)]
        assert sum(same_pair(h, whole) for h in held) == 1 and sum(not h[1].any() for h in held) == P - 1


# ---- (c) view_frame ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 13, 130])
def test_view_frame_properties(N):
    eps = np.finfo(np.float64).eps
    for (d, up) in VC.DIRECTIONS + [((0, 0, 1), (0, 1, 0)), ((0.3, -7.0, 1e-3), (0, 0, 1))]:
        for (W, H), step in zip(VC.FIXED_IMAGES + [VC.big_image(N)], VC.STEPS * 3):
            fr = VR.view_frame(N, d, up, W, H, step, 2.0)
            pix = np.sqrt(3.0) * N / max(W, H)
            r, u, dn = fr.du / pix, fr.dv / pix, fr.step / step
            for v in (r, u, dn):
                assert abs(VR._len(v) - 1.0) <= 2 * eps
            assert abs(np.dot(r, dn)) <= 4 * eps and abs(np.dot(u, dn)) <= 4 * eps and abs(np.dot(r, u)) <= 4 * eps
            # the centre ray (pixel ((W-1)/2, (H-1)/2), fractional for even extents) passes through c halfway
            L = np.sqrt(3.0) * N
            mid = fr.origin + fr.du * ((W - 1) / 2.0) + fr.dv * ((H - 1) / 2.0) + dn * (L / 2)
            assert np.max(np.abs(mid - (N + 1) / 2.0)) <= 8 * eps * (2 * N + 2)
            assert (fr.samples - 1) * step <= L < fr.samples * step  # the samples cover the sphere's diameter
            assert fr.sigma == 2.0 * step and fr.width == W and fr.height == H


# ---- (d) the conditions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", VC.SIZES)
def test_conditions_hold(N, dtype):
    for c in VC.cases_of(N, dtype):
        VC.check_conditions(c, *VC.reference(c))


def test_the_edge_frame_has_samples_on_the_box_face():
    for N in (5, 13):
        for dtype in VC.DTYPES:
            fr = VC.edge_frame(N)
            p = VR.position(fr, np.dtype(dtype).type, 0)
            assert (p[0][:, -1] == N + 0.5).all() and (p[1][-1, :] == N + 0.5).all()
            assert VR.visit_counts(N, dtype, fr).min() == N


# ---- (e) wrong variants --------------------------------------------------------------------------------------------
def accumulated(fr, T, n):
    """p += ds, n times, instead of o' + T(n) ds."""
    p = VR.position(fr, T, 0)
    for _ in range(n):
        p = [(x + T(fr.step[c])).astype(T) for c, x in enumerate(p)]
    return p


def rebracketed(fr, T, n):
    """((o + T(n) ds) + T(a) du) + T(b) dv."""
    a = np.arange(fr.width).astype(T)[None, :]
    b = np.arange(fr.height).astype(T)[:, None]
    return [(((T(fr.origin[c]) + T(n) * T(fr.step[c])) + a * T(fr.du[c])) + b * T(fr.dv[c])).astype(T) for c in range(3)]


def half_open(N, T, p):
    return VR.visited(N, T, p, half_open=True)


OBLIQUE = ("random", 13, np.float32, 0, 0.5, (16, 13), True)  # the (N+3) x N case of direction (1,2,3)
SINGLE = {
    "position-accumulated": (OBLIQUE, dict(position=accumulated)),
    "position-bracketed-from-the-step": (OBLIQUE, dict(position=rebracketed)),
    "unvisited-samples-clamped-into-the-box": (OBLIQUE, dict(clamp_unvisited=True)),
    "half-open-box": ("edge", dict(visited=half_open)),
    "n-from-1": ("axis", dict(order="from1")),
    "du-dv-swapped": (OBLIQUE, "swap"),
    "back-to-front": (OBLIQUE, dict(order="reversed")),
    "emission-at-the-nearest-cell": (OBLIQUE, dict(nearest_emit=True)),
    "Tr-before-C": (OBLIQUE, dict(tr_first=True)),
}


@pytest.mark.parametrize("name", list(SINGLE), ids=[
    f"{k}--caught-by-{'test_axis_frames[N13-f32]' if v[0] in ('edge', 'axis') else 'test_every_case:' + VC.case_id(VC.Case(*v[0]))}"
    for k, v in SINGLE.items()])
def test_wrong_variant_differs(name):
    where, how = SINGLE[name]
    if where not in ("edge", "axis"):
        assert VC.Case(*where) in VC.CASES, "the case named is not one the GPU test runs"
    if where == "edge":
        dens, emit, _ = VC.inputs("shells", 13, np.float32)
        fr = VC.edge_frame(13)
    elif where == "axis":
        dens, emit, sigma = VC.inputs("random", 13, np.float32)
        fr = VR.axis_frame(13, 2, 0, sigma)
    else:
        c = VC.Case(*where)
        dens, emit, _ = VC.inputs(c.family, c.N, c.dtype)
        fr = VC.case_frame(c)
    want = VR.render_view(dens, emit, fr)
    if how == "swap":
        got = VR.render_view(dens, emit, fr._replace(du=fr.dv, dv=fr.du))
    else:
        how = dict(how)
        if how.get("order") == "from1":
            how["order"] = range(1, fr.samples + 1)
        elif how.get("order") == "reversed":
            how["order"] = range(fr.samples - 1, -1, -1)
        got = VR.render_view(dens, emit, fr, **how)
    assert not same_pair(got, want), f"{name} equals the reference"


def owner_above(z, vis):
    return VR.owner_k(z, vis) + 1


CHAIN = {
    "carry-reset-at-a-slab": dict(hand_on=lambda st, dt: (np.zeros_like(st[0]), np.ones_like(st[1]))),
    "only-Tr-carried": dict(hand_on=lambda st, dt: (np.zeros_like(st[0]), st[1])),
    "owner-by-k0-plus-1": dict(owner=owner_above),
    "chain-upwards-iff-step_z-not-positive": dict(high="inverted"),
}


@pytest.mark.parametrize("name", list(CHAIN), ids=[f"{k}--caught-by-test_every_decomposition[N34-P2-copy-f32]" for k in CHAIN])
def test_wrong_chain_differs(name):
    N, P, dtype = 34, 2, np.float32
    dens, emit, _ = VC.inputs("random", N, dtype)
    fr = VC.frame(N, 0, *VC.CHAIN_VIEW)
    want = VR.render_view(dens, emit, fr)
    how = dict(CHAIN[name])
    if how.get("high") == "inverted":
        how["high"] = bool(np.float32(fr.step[2]) > 0)  # upwards iff step_z <= 0
    assert same_pair(VR.render_view_slabs(dens, emit, fr, P), want)
    assert not same_pair(VR.render_view_slabs(dens, emit, fr, P, **how), want), f"{name} equals the reference"
