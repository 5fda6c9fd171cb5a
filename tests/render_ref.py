"""docs/SPEC.md §12 in numpy: axis-aligned volume rendering and light marching. A ray is walked cell by cell in the
order the SPEC fixes (a Python loop over the N steps), all N x N rays of an image at once (numpy over the image), every
value in the dtype of the density, every expression bracketed as written. Arrays are (N+2)^3, indexed [k, j, i].

render_slabs is the decomposition of §12 spelt out: the slabs of a k-ray visited in order, each starting from the image
pair the one before it left. With the pair handed on intact it is `render` operation for operation, which is why the
bits do not depend on P; it exists so that a carry that is NOT handed on intact (tests/test_render_ref.py) has something
to be told from."""
import numpy as np

import stable_ref as S3

AXES = {"i": 0, "j": 1, "k": 2}


def scalar(N, dtype, sigma):
    """s = T(sigma) * h, h = T(1) / T(N) (SPEC §2)."""
    T = np.dtype(dtype).type
    return T(sigma) * (T(1) / T(N))


def opacity(s, d):
    """a = (t > 0) ? ((t < 1) ? t : 1) : 0 with t = s * d: NaN and negative densities give +0, t >= 1 gives 1."""
    T = d.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        t = s * d
        return np.where(t > 0, np.where(t < 1, t, T(1)), T(0)).astype(d.dtype)


def cells(x, axis, idx):
    """The interior cells of index idx along `axis` as an image [b - 1, a - 1] over the two remaining axes a < b."""
    N = x.shape[0] - 2
    inner = slice(1, N + 1)
    return x[(inner, inner, idx) if axis == 0 else (inner, idx, inner) if axis == 1 else (idx, inner, inner)]


def visit_order(N, from_high, lo=1, hi=None):
    """The indices lo .. hi (default 1 .. N) in the order a ray of direction from_high visits them."""
    hi = N if hi is None else hi
    return range(hi, lo - 1, -1) if from_high else range(lo, hi + 1)


def start(N, dtype):
    return np.zeros((N, N), dtype), np.ones((N, N), dtype)


def march(dens, emit, axis, order, s, state):
    """Applies the cells `order` to the state (C, Tr): C first, from the old Tr."""
    C, Tr = state
    T = dens.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        for idx in order:
            a = opacity(s, cells(dens, axis, idx))
            C = C + (Tr * a) * cells(emit, axis, idx) if emit is not None else C + Tr * a
            Tr = Tr * (T(1) - a)
    return C, Tr


def render(dens, emit, axis, from_high, sigma):
    """(C, Tr): the final colour and transmittance of every ray, two (N, N) arrays [b - 1, a - 1]."""
    N = dens.shape[0] - 2
    s = scalar(N, dens.dtype, sigma)
    return march(dens, emit, axis, visit_order(N, from_high), s, start(N, dens.dtype))


def slab_images(dens, emit, axis, from_high, sigma, P, rank):
    """What the context that holds the slabs `rank` (an iterable of slab indices of P) reads back after a render of the
    whole grid: its pixels of (C, Tr), zeros elsewhere. i and j views: the pixel rows b = k of its planes; a k view: the
    whole image where the rays leave the grid, nothing elsewhere."""
    N = dens.shape[0] - 2
    nzl = N // P
    C, Tr = render(dens, emit, axis, from_high, sigma)
    keep = np.zeros((N, N), bool)
    for g in rank:
        if axis < 2:
            keep[g * nzl:(g + 1) * nzl] = True
        elif g == (0 if from_high else P - 1):
            keep[:] = True
    return np.where(keep, C, 0).astype(dens.dtype), np.where(keep, Tr, 0).astype(dens.dtype)


def render_slabs(dens, emit, from_high, sigma, P, hand_on=lambda state, dtype: state):
    """A k view over P slabs of N / P planes: the chain of §12. hand_on(state, dtype) is what crosses a slab boundary
    (the identity: the pair intact)."""
    N = dens.shape[0] - 2
    nzl = N // P
    s = scalar(N, dens.dtype, sigma)
    state = start(N, dens.dtype)
    slabs = range(P - 1, -1, -1) if from_high else range(P)
    for n, g in enumerate(slabs):
        if n:
            state = hand_on(state, dens.dtype)
        state = march(dens, emit, 2, visit_order(N, from_high, g * nzl + 1, (g + 1) * nzl), s, state)
    return state


def light(dens, axis, from_high, sigma):
    """dst: the Tr of the ray before each cell is applied (exactly 1 on the first cell visited), then set_bnd(0, dst)."""
    N = dens.shape[0] - 2
    T = dens.dtype.type
    s = scalar(N, dens.dtype, sigma)
    dst = np.zeros_like(dens)
    Tr = np.ones((N, N), dens.dtype)
    for idx in visit_order(N, from_high):
        cells(dst, axis, idx)[...] = Tr
        Tr = Tr * (T(1) - opacity(s, cells(dens, axis, idx)))
    S3.set_bnd(0, dst)
    return dst


def quantise(C):
    """The 16-bit grey values of the driver's PGM: (int)(min(max(C, 0), 1) * 65535 + 0.5) in double, NaN -> 0."""
    c = np.asarray(C, np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(c > 0, np.where(c < 1, c, 1.0), 0.0)
    return (c * 65535.0 + 0.5).astype(np.int64).astype(">u2")


def pgm_bytes(C):
    """The file the driver writes for the image C [b - 1, a - 1]: binary P5, maxval 65535, big-endian, the row with the
    highest b first."""
    q = quantise(C)[::-1]
    return b"P5\n%d %d\n65535\n" % (q.shape[1], q.shape[0]) + q.tobytes()
