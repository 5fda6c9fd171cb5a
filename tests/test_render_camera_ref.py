"""The numpy reference of docs/SPEC.md §14 (tests/render_camera_ref.py) against closed cases of the camera, the
identities of §14.1, the conditions the cases of tests/camera_cases.py have to meet, and wrong variants of the reference:
each is a way a kernel, a chain or a frame could plausibly go wrong, and each is shown to differ from the reference on a
named case — the GPU case of tests/test_render_camera_gpu.py that would catch a library that computed it. No GPU
needed."""
import numpy as np
import pytest

import camera_cases as CC
import render_camera_ref as CR
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


# ---- (a) the conditions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", CC.ALL_SIZES)
def test_conditions_hold(N, dtype):
    for c in CC.cases_of(N, dtype):
        C, Tr = CC.reference(c)
        print(CC.case_id(c), "visited %d partial %d Tr=0 %d NaN C %d NaN Tr %d missed %d" % CC.figures(c, C, Tr))
        CC.check_conditions(c, C, Tr)


def test_the_table_covers_what_it_says():
    for N in CC.SIZES:
        assert {c.camera for c in CC.CASES if c.N == N} == set(CC.CAMERAS), N
        for dtype in CC.DTYPES:
            assert CC.cases_of(N, dtype)
    assert {c.step for c in CC.CASES} == set(CC.STEPS)
    assert {c.family for c in CC.CASES} == set(CC.FAMILIES)
    for image in CC.FIXED_IMAGES:
        assert any(c.image == image for c in CC.CASES), image
    assert [c.N for c in CC.CASES].count(CC.ONE_FRAME) == 2
    for c in CC.CASES:
        if c.camera == "K":
            assert c.image[0] % 2 and c.image[1] % 2, CC.case_id(c)
    # the passes the cameras are named for, on the image of the conditions and on the image of the chain
    for N in (13, 34, 70):
        for image in (CC.big_image(N), CC.CHAIN_VIEW[1]):
            for dtype in CC.DTYPES:
                got = {cam: CR.passes(CC.frame(N, cam, 0.5, image), dtype) for cam in CC.CAMERAS}
                assert got == {"A": CR.BOTH, "B": CR.BOTH, "C": CR.BOTH, "U": CR.UP, "D": CR.DOWN, "K": CR.UP}, (N, image, got)


# ---- (b) camera_frame ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 13, 130])
def test_camera_frame_properties(N):
    eps = np.finfo(np.float64).eps
    for cam in CC.CAMERAS:
        eye, target, up, tan = CC.camera(N, cam)
        eye, target = np.array(eye), np.array(target)
        for (W, H), step in zip(CC.FIXED_IMAGES + [CC.big_image(N)], CC.STEPS * 3):
            fr = CR.camera_frame(N, eye, target, up, tan, W, H, step, 3.0)
            d = (target - eye) / VR._len(target - eye)
            dc = float(np.dot((N + 1) / 2.0 - eye, d))
            R = np.sqrt(3.0) * N / 2.0
            t0 = max(dc - R, 0.0)
            scale = 8 * eps * (4 * N + 4)
            assert fr.sigma == 3.0 and (fr.width, fr.height) == (W, H)
            assert (fr.samples - 1) * step <= (dc + R) - t0 + scale and (dc + R) - t0 < fr.samples * step + scale
            for a, b in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), ((W - 1) / 2.0, (H - 1) / 2.0)):
                r = fr.step + a * fr.step_du + b * fr.step_dv
                o = fr.origin + a * fr.du + b * fr.dv
                # sample n lies at depth t0 + n step along d, and on the line through the eye
                assert abs(np.dot(r, d) - step) <= scale and abs(np.dot(o - eye, d) - t0) <= scale
                assert np.max(np.abs(np.cross(o - eye, r))) <= scale * (4 * N + 4) * max(step, 1.0) * 4
            mid = fr.step + (W - 1) / 2.0 * fr.step_du + (H - 1) / 2.0 * fr.step_dv
            assert np.max(np.abs(mid - d * step)) <= scale  # the centre ray looks along d
            # the vertical field of view: the pixel rows span 2 tan at depth 1
            top = fr.step_dv * H / step
            assert abs(VR._len(top) - 2.0 * tan) <= 16 * eps * max(1.0, 2 * tan)
            if cam == "A":  # the eye is inside the bounding sphere: every ray starts at the eye
                assert t0 == 0.0 and (fr.origin == eye).all() and not fr.du.any() and not fr.dv.any()


def test_camera_k_is_exact():
    """Looking along +k from straight below: d = (0, 0, 1), r = (-1, 0, 0), u = (0, 1, 0) without a rounding, and with
    odd extents the centre pixel's step vector is exactly (0, 0, step)."""
    for N in (5, 13, 34):
        eye, target, up, tan = CC.camera(N, "K")
        for (W, H), step in (((7, 5), 0.5), ((9, 17), 1.0), ((65, 3), 1.7)):
            fr = CR.camera_frame(N, eye, target, up, tan, W, H, step, 1.0)
            pp = (2.0 * tan) / H
            assert (fr.step_du == np.array([-1.0, 0, 0]) * (pp * step)).all() and (fr.step_dv == np.array([0, 1.0, 0]) * (pp * step)).all()
            for dtype in CC.DTYPES:
                r = CR.direction(fr, dtype)
                ca, cb = (W - 1) // 2, (H - 1) // 2
                assert r[2][cb, ca] == dtype(step)
                if dtype is np.float64:  # (in fp32 the products T(a) * T(dsu) need not cancel T(ds))
                    assert r[0][cb, ca] == 0 and r[1][cb, ca] == 0
            assert CR.passes(fr, np.float32) == CR.UP


def test_camera_frame_refuses_what_the_spec_names():
    N, c = 8, 4.5
    good = dict(N=N, eye=(c, c, -10.0), target=(c, c, c), up=(0, 1, 0), tan_half_fov=0.5, width=4, height=5, step=1.0, sigma=1.0)
    assert CR.camera_frame(**good) is not None
    for bad in (dict(target=good["eye"]), dict(up=(0, 0, 1)), dict(up=(0, 0, -3)), dict(tan_half_fov=0.0),
                dict(tan_half_fov=-1.0), dict(step=0.0), dict(step=-0.5), dict(eye=(c, c, 40.0), target=(c, c, 80.0)),
                dict(step=1e-4)):
        assert CR.camera_frame(**{**good, **bad}) is None, bad
    fr = CR.camera_frame(**{**good, "step": (np.sqrt(3.0) * N) / 65535.5})
    assert fr is not None and fr.samples == 65536


# ---- (c) the corner rule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=DTYPE_IDS)
def test_corner_rule_agrees_with_all_pixels(dtype):
    """r_z is monotone in a and in b, so the four corners decide; checked against every pixel of random cameras, and
    the monotonicity itself along every row and column."""
    rng = np.random.RandomState(1400)
    seen = set()
    for n in range(300):
        N = (5, 34, 130)[n % 3]
        c = (N + 1) / 2.0
        eye = c + N * rng.uniform(-1.5, 1.5, 3)
        target = c + N * rng.uniform(-0.5, 0.5, 3)
        if n % 4 == 0:
            target[2] = eye[2]  # a level camera: r_z changes sign across the rows
        W, H = (CC.FIXED_IMAGES + [(37, 34), (129, 2)])[n % 8]
        fr = CR.camera_frame(N, eye, target, (0, 0, 1), rng.uniform(0.05, 2.0), W, H, (0.5, 1.0, 1.7)[n % 3], 1.0)
        if fr is None:
            continue
        rz = CR.direction(fr, dtype)[2]
        for axis in (0, 1):
            diff = np.diff(rz, axis=axis)
            assert (diff >= 0).all() or (diff <= 0).all(), (n, axis)
        down = CR.is_down(fr, dtype)
        want = CR.DOWN if down.all() else (CR.BOTH if down.any() else CR.UP)
        assert CR.passes(fr, dtype) == want, n
        seen.add(want)
    assert seen == {CR.UP, CR.DOWN, CR.BOTH}


# ---- (d) the identities of §14.1 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", VC.AXIS_SIZES)
def test_identities(N, dtype):
    dens, emit, sigma = CC.inputs("random", N, dtype)
    for axis, high in RC.VIEWS:  # step_du = step_dv = 0, |r| = 1: the axis render of §12 and the view of §13
        fr = VR.axis_frame(N, axis, high, sigma)
        for e in (emit, None):
            got = CR.render_camera(dens, e, CR.of_view(fr))
            assert same_pair(got, RR.render(dens, e, axis, high, sigma)), (N, axis, high)
            assert same_pair(got, VR.render_view(dens, e, fr)), (N, axis, high)
    for axis, high in RC.VIEWS:  # every second cell centre: |r| = 2 doubles the opacity scalar, exactly
        fr = VR.axis_frame(N, axis, high, 2 * sigma)
        fr = fr._replace(step=fr.step * 2.0, samples=max(N // 2, 1))
        assert same_pair(CR.render_camera(dens, emit, CR.of_view(fr, sigma)), VR.render_view(dens, emit, fr)), (N, axis, high)
    zero = np.zeros_like(dens)
    for cam in CC.CAMERAS:
        fr = CC.frame(N, cam, 0.5, (9, 17))
        assert same_pair(CR.render_camera(zero, emit, fr), VR.start(fr, dtype)), cam
    dens, emit, _ = CC.inputs("shells", N, dtype)
    fr = VC.edge_frame(N)
    assert same_pair(CR.render_camera(dens, emit, CR.of_view(fr)), VR.render_view(dens, emit, fr))


# ---- (e) the chain -------------------------------------------------------------------------------------------------
def crossing(N, dtype, fr, P):
    """(up pixels, down pixels) with visited samples in two or more slabs."""
    many = CR.slabs_crossed(N, dtype, fr, P) >= 2
    down = CR.is_down(fr, np.dtype(dtype).type)
    return int(np.count_nonzero(many & ~down)), int(np.count_nonzero(many & down))


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N,P,transport", CC.DECOMPOSED, ids=[f"N{n}-P{p}" for n, p, _ in CC.DECOMPOSED])
def test_the_two_pass_chain_equals_the_undecomposed_render(N, P, transport, dtype):
    dens, emit, _ = CC.inputs("random", N, dtype)
    ups = downs = 0
    for cam in CC.CHAIN_CAMERAS:
        fr = CC.frame(N, cam, *CC.CHAIN_VIEW)
        whole = CR.render_camera(dens, emit, fr)
        assert same_pair(CR.render_camera_slabs(dens, emit, fr, P), whole), (N, P, cam)
        held = [CR.held_pixels(dens, emit, fr, P, [g]) for g in range(P)]
        assert sum(same_pair(h, whole) for h in held) == 1 and sum(not h[1].any() for h in held) == P - 1
        what = CR.passes(fr, dtype)
        assert same_pair(held[P - 1 if what == CR.UP else 0], whole), cam
        if cam in ("A", "C"):
            assert what == CR.BOTH
            u, d = crossing(N, dtype, fr, P)
            print(f"N={N} P={P} camera {cam}: {u} up pixels and {d} down pixels cross a slab boundary")
            ups, downs = ups + u, downs + d
    assert ups >= 8 and downs >= 8, (ups, downs)


# ---- (f) wrong variants --------------------------------------------------------------------------------------------
def r_rebracketed(fr, T):
    """(ds + T(b) dsv) + T(a) dsu."""
    a, b = CR._ab(fr, T)
    return [((T(fr.step[c]) + b * T(fr.step_dv[c])) + a * T(fr.step_du[c])).astype(T) for c in range(3)]


def r_folded(fr, T, n, direction):
    """((base + T(n) ds) + (T(n) T(a)) dsu) + (T(n) T(b)) dsv: r never formed."""
    a, b = CR._ab(fr, T)
    return [(((((T(fr.origin[c]) + a * T(fr.du[c])) + b * T(fr.dv[c])) + T(n) * T(fr.step[c])) + (T(n) * a) * T(fr.step_du[c])) +
             (T(n) * b) * T(fr.step_dv[c])).astype(T) for c in range(3)]


def accumulated(fr, T, n, direction):
    """p += r, n times, instead of base + T(n) r."""
    p, r = CR.position(fr, T, 0), direction(fr, T)
    for _ in range(n):
        p = [(x + r[c]).astype(T) for c, x in enumerate(p)]
    return p


def s_without_length(fr, N, T, r):
    return np.full(r[0].shape, RR.scalar(N, T, fr.sigma), T)


def length_bracketed_from_the_right(r):
    return np.sqrt(r[0] * r[0] + (r[1] * r[1] + r[2] * r[2]))


def s_length_right(fr, N, T, r):
    return CR.scalar(fr, N, T, r, length=length_bracketed_from_the_right)


OBLIQUE = ("random", 13, np.float32, "C", 0.5, (16, 13), False)  # the (N+3) x N case of camera C
SINGLE = {
    "r-bracketed-from-dsv": dict(direction=r_rebracketed),
    "r-folded-into-the-position": dict(position=r_folded),
    "position-accumulated": dict(position=accumulated),
    "s-without-the-length-of-r": dict(scalar=s_without_length),
    "length-of-r-bracketed-from-the-right": dict(scalar=s_length_right),
}


@pytest.mark.parametrize("name", list(SINGLE), ids=[f"{k}--caught-by-test_every_case:{CC.case_id(CC.Case(*OBLIQUE))}" for k in SINGLE])
def test_wrong_variant_differs(name):
    c = CC.Case(*OBLIQUE)
    assert c in CC.CASES, "the case named is not one the GPU test runs"
    dens, emit, _ = CC.inputs(c.family, c.N, c.dtype)
    got = CR.render_camera(dens, None, CC.case_frame(c), **SINGLE[name])
    assert not same_pair(got, CC.reference(c)), f"{name} equals the reference"


def centre_rule(fr, T, direction=CR.direction):
    down = CR.is_down(fr, T, direction)
    return CR.DOWN if down[fr.height // 2, fr.width // 2] else CR.UP


def down_or_level(fr, T):
    with np.errstate(invalid="ignore"):
        return CR.direction(fr, T)[2] <= T(0)


CHAIN = {  # name: (camera, keywords of render_camera_slabs)
    "mixed-frame-as-one-upward-pass": ("C", dict(single_up=True)),
    "pass-chosen-by-the-centre-pixel": ("A", dict(rule=centre_rule)),
    "down-pass-restarts-from-nothing": ("A", dict(restart_down=True)),
    "down-pass-applies-the-up-pixels-again": ("A", dict(mask_down=False)),
}
CHAIN_CASE = (34, 17, np.float32)


@pytest.mark.parametrize("name", list(CHAIN), ids=[f"{k}--caught-by-test_every_decomposition[N34-P17-rccl-self-f32]" for k in CHAIN])
def test_wrong_chain_differs(name):
    N, P, dtype = CHAIN_CASE
    assert (N, P, "rccl-self") in CC.DECOMPOSED
    cam, how = CHAIN[name]
    assert cam in CC.CHAIN_CAMERAS
    dens, emit, _ = CC.inputs("random", N, dtype)
    fr = CC.frame(N, cam, *CC.CHAIN_VIEW)
    want = CR.render_camera(dens, emit, fr)
    assert same_pair(CR.render_camera_slabs(dens, emit, fr, P), want)
    assert not same_pair(CR.render_camera_slabs(dens, emit, fr, P, **how), want), f"{name} equals the reference"


def level_frame(N):
    """Rays that stay inside a slab (direction (1,1,0) of §13) as a camera frame: r_z = +0 in every pixel."""
    return CR.of_view(VC.frame(N, 2, *VC.CHAIN_VIEW), VC.SIGMA)


def test_split_at_level_rays_differs__caught_by_test_camera_passes():
    """`down iff r_z <= 0` renders the same image and names another pass (and another context for the image)."""
    N, P, dtype = CHAIN_CASE
    fr = level_frame(N)
    assert not CR.direction(fr, dtype)[2].any()
    assert CR.passes(fr, dtype) == CR.UP
    wrong = lambda fr, T: CR.corner_rule(fr, T) if CR.direction(fr, T)[2].any() else CR.DOWN  # noqa: E731
    assert CR.passes(fr, dtype, rule=wrong) == CR.DOWN
    assert CR.last_slab(fr, dtype, P) == P - 1 and CR.last_slab(fr, dtype, P, rule=wrong) == 0
    dens, emit, _ = CC.inputs("random", N, dtype)
    assert same_pair(CR.render_camera_slabs(dens, emit, fr, P, down_of=down_or_level), CR.render_camera(dens, emit, fr))


def test_image_on_the_last_slab_of_a_mixed_frame_differs__caught_by_test_every_decomposition():
    """A library that read a mixed frame's image from slab P - 1 would return the pair the upward pass left there."""
    N, P, dtype = CHAIN_CASE
    dens, emit, _ = CC.inputs("random", N, dtype)
    fr = CC.frame(N, "A", *CC.CHAIN_VIEW)
    whole = CR.render_camera(dens, emit, fr)
    assert same_pair(CR.held_pixels(dens, emit, fr, P, [0]), whole)
    assert not same_pair(CR.held_pixels(dens, emit, fr, P, [0], mixed_ends_on_top=True), whole)
    down = CR.is_down(fr, dtype)
    state = VR.start(fr, dtype)
    for g in range(P):  # what slab P - 1 holds after the upward pass
        state = CR.render_camera(dens, emit, fr, krange=(g * (N // P) + 1, (g + 1) * (N // P)), state=state, only=~down)
    assert not same_pair(state, whole)
