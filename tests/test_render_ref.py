"""The numpy reference of docs/SPEC.md §12 (tests/render_ref.py) against the closed forms of §12.1, the conditions the
inputs of tests/render_cases.py have to meet, and wrong variants of the reference: each is a way a kernel or a carry
could plausibly go wrong, and each is shown to differ from the reference on a named case — the GPU case of
tests/test_render_gpu.py that would catch a library that computed it. No GPU needed."""
import numpy as np
import pytest

import render_cases as RC
import render_ref as RR

DTYPE_IDS = ["f32", "f64"]


def same_bits(a, b):
    uint = np.uint32 if a.dtype == np.float32 else np.uint64
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all((a.view(uint) == b.view(uint)) | both_nan))


# ---- §12.1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", RC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", RC.SIZES)
def test_closed_forms(N, dtype):
    T = np.dtype(dtype).type
    mant = np.finfo(dtype).nmant + 1
    eps = np.finfo(dtype).eps
    for axis, high in RC.VIEWS:
        dens, emit, sigma = RC.closed("zero", N, dtype)
        for e in (emit, None):
            C, Tr = RR.render(dens, e, axis, high, sigma)
            assert same_bits(C, np.zeros((N, N), dtype)) and same_bits(Tr, np.ones((N, N), dtype))
        assert same_bits(RR.light(dens, axis, high, sigma), np.ones_like(dens))

        dens, emit, sigma = RC.closed("half", N, dtype)
        C, Tr = RR.render(dens, None, axis, high, sigma)
        if N <= mant:
            assert same_bits(Tr, np.full((N, N), T(2.0) ** -N, dtype))
            assert same_bits(C, np.full((N, N), T(1) - T(2.0) ** -N, dtype))
        lit = RR.light(dens, axis, high, sigma)
        for n, idx in enumerate(RR.visit_order(N, high)):  # the exclusive transmittance: 2^-n in front of the n-th cell
            if n < 120:
                assert same_bits(np.ascontiguousarray(RR.cells(lit, axis, idx)), np.full((N, N), T(2.0) ** -n, dtype))

        dens, emit, sigma = RC.closed("opaque", N, dtype, axis, high)
        C, Tr = RR.render(dens, emit, axis, high, sigma)
        assert same_bits(Tr, np.zeros((N, N), dtype))
        assert same_bits(C, np.ascontiguousarray(RR.cells(emit, axis, N if high else 1)))

        dens, emit, sigma = RC.inputs("random", N, dtype)
        C, Tr = RR.render(dens, None, axis, high, sigma)
        assert float(np.max(np.abs(C - (T(1) - Tr)))) <= 2 * N * eps  # no emission: C = 1 - Tr up to rounding
        lit = RR.light(dens, axis, high, sigma)
        last = 1 if high else N
        a = RR.opacity(RR.scalar(N, dtype, sigma), RR.cells(dens, axis, last))
        assert same_bits((RR.cells(lit, axis, last) * (T(1) - a)).astype(dtype), Tr)
        assert same_bits(np.ascontiguousarray(RR.cells(lit, axis, N if high else 1)), np.ones((N, N), dtype))


def test_opacity_select_form():
    for dtype in RC.DTYPES:
        T = np.dtype(dtype).type
        d = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 0.25, 1.0, 1.5, np.inf], dtype)
        a = RR.opacity(T(1), d)
        assert same_bits(a, np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.25, 1.0, 1.0, 1.0], dtype))
        assert not np.signbit(a).any()  # a transparent cell is +0


def test_quantisation():
    C = np.array([[np.nan, -1.0, 0.0, 0.5], [1.0, 2.0, np.inf, 1.0 / 65535.0]], np.float32)
    q = RR.quantise(C)
    assert q.tolist() == [[0, 0, 0, 32768], [65535, 65535, 65535, 1]]
    raw = RR.pgm_bytes(C)
    assert raw.startswith(b"P5\n4 2\n65535\n") and len(raw) == 13 + 16
    assert raw[13:15] == b"\xff\xff" and raw[13 + 8 + 6:13 + 8 + 8] == b"\x80\x00"  # the row with the highest b first


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", RC.SIZES)
def test_conditions_hold(N, dtype):
    """The conditions of render_cases on the reference result of every family, view and size."""
    for family in RC.FAMILIES:
        dens, emit, sigma = RC.inputs(family, N, dtype)
        for axis, high in RC.VIEWS:
            for e in (emit, None):
                RC.check_conditions(family, N, dens, *RR.render(dens, e, axis, high, sigma))


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N,P,transport", RC.DECOMPOSED)
def test_the_chain_is_the_ray(N, P, transport, dtype):
    """render_slabs with the pair handed on intact is render, bit for bit, and the slabs' pixels tile the image."""
    dens, emit, sigma = RC.inputs("random", N, dtype)
    for high in (0, 1):
        C, Tr = RR.render(dens, emit, 2, high, sigma)
        kC, kTr = RR.render_slabs(dens, emit, high, sigma, P)
        assert same_bits(kC, C) and same_bits(kTr, Tr)
    for axis, high in RC.VIEWS:
        C, Tr = RR.render(dens, emit, axis, high, sigma)
        total = np.zeros_like(C)
        for g in range(P):
            sC, sTr = RR.slab_images(dens, emit, axis, high, sigma, P, [g])
            total = total + sC
        assert same_bits(total + 0, C + 0)


# ---- wrong variants ------------------------------------------------------------------------------------------------
def variant_render(dens, emit, axis, high, sigma, order=None, colour="spec", first="C", alpha="select"):
    """render with one thing changed. order: the indices visited; colour: how C's increment is bracketed; first: which
    of C and Tr is updated first; alpha: how the opacity is clamped."""
    N = dens.shape[0] - 2
    T = dens.dtype.type
    s = RR.scalar(N, dens.dtype, sigma)
    C, Tr = RR.start(N, dens.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for idx in (RR.visit_order(N, high) if order is None else order):
            d = RR.cells(dens, axis, idx)
            if alpha == "select":
                a = RR.opacity(s, d)
            elif alpha == "minmax":  # hardware min / max: a NaN operand gives the other one, here 1
                a = np.where(np.isnan(s * d), T(1), RR.opacity(s, d)).astype(dens.dtype)  # max(min(NaN, 1), 0) = 1
            else:  # "unclamped": t >= 1 passes through
                t = s * d
                a = np.where(t > 0, t, T(0)).astype(dens.dtype)
            e = RR.cells(emit, axis, idx)
            if first == "Tr":
                Tr = Tr * (T(1) - a)
            C = C + Tr * (a * e) if colour == "a*e" else C + (Tr * a) * e
            if first == "C":
                Tr = Tr * (T(1) - a)
    return C, Tr


def variant_light(dens, axis, high, sigma, inclusive):
    N = dens.shape[0] - 2
    T = dens.dtype.type
    s = RR.scalar(N, dens.dtype, sigma)
    dst = np.zeros_like(dens)
    Tr = np.ones((N, N), dens.dtype)
    for idx in RR.visit_order(N, high):
        if not inclusive:
            RR.cells(dst, axis, idx)[...] = Tr
        Tr = Tr * (T(1) - RR.opacity(s, RR.cells(dens, axis, idx)))
        if inclusive:
            RR.cells(dst, axis, idx)[...] = Tr
    RR.S3.set_bnd(0, dst)
    return dst


def composite_afterwards(dens, emit, high, sigma, P):
    """Per-slab partial images, each from (0, 1), composited in visit order afterwards: C = C + Tr * C_s; Tr = Tr * Tr_s.
    Equal to the ray in exact arithmetic, another rounding sequence in T."""
    N = dens.shape[0] - 2
    nzl = N // P
    s = RR.scalar(N, dens.dtype, sigma)
    C, Tr = RR.start(N, dens.dtype)
    for g in (range(P - 1, -1, -1) if high else range(P)):
        sC, sTr = RR.march(dens, emit, 2, RR.visit_order(N, high, g * nzl + 1, (g + 1) * nzl), s, RR.start(N, dens.dtype))
        C = C + Tr * sC
        Tr = Tr * sTr
    return C, Tr


RESET = lambda state, dtype: RR.start(state[0].shape[0], dtype)
TR_ONLY = lambda state, dtype: (np.zeros_like(state[0]), state[1])

# (what is wrong, the case of tests/test_render_gpu.py that catches it: test id and view, how the variant is computed)
N_RAY, N_SLAB, P_SLAB = 13, 34, 2
MUTANTS = [
    ("back-to-front order", "test_every_view_at_every_size[N13-f32] random j+",
     lambda d, e: variant_render(d, e, 1, 0, RC.SIGMA, order=RR.visit_order(N_RAY, 1)), (1, 0)),
    ("C + Tr * (a * e)", "test_every_view_at_every_size[N13-f32] random i+",
     lambda d, e: variant_render(d, e, 0, 0, RC.SIGMA, colour="a*e"), (0, 0)),
    ("Tr updated before C", "test_every_view_at_every_size[N13-f32] random k-",
     lambda d, e: variant_render(d, e, 2, 1, RC.SIGMA, first="Tr"), (2, 1)),
    ("t >= 1 not clamped", "test_every_view_at_every_size[N13-f32] random k+",
     lambda d, e: variant_render(d, e, 2, 0, RC.SIGMA, alpha="unclamped"), (2, 0)),
    ("from_high starting at N + 1", "test_every_view_at_every_size[N13-f32] shells i-",
     lambda d, e: variant_render(d, e, 0, 1, RC.SIGMA, order=range(N_RAY + 1, 1, -1)), (0, 1)),
    ("from_high stopping at 2", "test_every_view_at_every_size[N13-f32] random i-",
     lambda d, e: variant_render(d, e, 0, 1, RC.SIGMA, order=range(N_RAY, 1, -1)), (0, 1)),
    ("shell cell read at the low end", "test_every_view_at_every_size[N13-f32] shells j+",
     lambda d, e: variant_render(d, e, 1, 0, RC.SIGMA, order=range(0, N_RAY + 1)), (1, 0)),
    ("shell cell read at the high end", "test_every_view_at_every_size[N13-f32] shells k+",
     lambda d, e: variant_render(d, e, 2, 0, RC.SIGMA, order=range(1, N_RAY + 2)), (2, 0)),
    ("the two pixel axes swapped", "test_every_view_at_every_size[N13-f32] random j+",
     lambda d, e: tuple(x.T.copy() for x in RR.render(d, e, 1, 0, RC.SIGMA)), (1, 0)),
]


@pytest.mark.parametrize("what,case,variant,view", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_wrong_rays_differ(what, case, variant, view):
    family = case.split("] ")[1].split()[0]
    dens, emit, sigma = RC.inputs(family, N_RAY, np.float32)
    C, Tr = RR.render(dens, emit, view[0], view[1], sigma)
    mC, mTr = variant(dens, emit)
    assert not (same_bits(mC, C) and same_bits(mTr, Tr)), f"{what} is the reference on {case}"


def test_hardware_min_max_differs_on_nan():
    """Opacity by v_min / v_max returns the non-NaN operand: a NaN density would be opaque, the SPEC says transparent.
    Caught by test_every_view_at_every_size[N13-f32] special (every view: the family plants NaN in dens)."""
    dens, emit, sigma = RC.inputs("special", N_RAY, np.float32)
    assert np.isnan(dens[RC.INNER]).any()
    for axis, high in RC.VIEWS:
        C, Tr = RR.render(dens, None, axis, high, sigma)
        mC, mTr = variant_render(dens, np.ones_like(dens), axis, high, sigma, alpha="minmax")
        assert not same_bits(mTr, Tr), (axis, high)


def test_inclusive_light_differs():
    """Caught by test_every_view_at_every_size[N13-f32] random (light, every view)."""
    dens, _, sigma = RC.inputs("random", N_RAY, np.float32)
    for axis, high in RC.VIEWS:
        assert not same_bits(variant_light(dens, axis, high, sigma, True), RR.light(dens, axis, high, sigma))
        assert same_bits(variant_light(dens, axis, high, sigma, False), RR.light(dens, axis, high, sigma))


@pytest.mark.parametrize("high", (0, 1))
def test_wrong_carries_differ(high):
    """Caught by test_every_view_on_every_decomposition[N34-P2-copy-f32] random k+ / k-."""
    dens, emit, sigma = RC.inputs("random", N_SLAB, np.float32)
    C, Tr = RR.render(dens, emit, 2, high, sigma)
    rC, rTr = RR.render_slabs(dens, emit, high, sigma, P_SLAB, hand_on=RESET)
    assert not same_bits(rTr, Tr) and not same_bits(rC, C), "the carry reset to (0, 1) at a slab boundary"
    tC, tTr = RR.render_slabs(dens, emit, high, sigma, P_SLAB, hand_on=TR_ONLY)
    assert same_bits(tTr, Tr) and not same_bits(tC, C), "only Tr carried"
    cC, cTr = composite_afterwards(dens, emit, high, sigma, P_SLAB)
    assert not (same_bits(cC, C) and same_bits(cTr, Tr)), "per-slab partial images composited afterwards"
