"""docs/SPEC.md §13 in numpy: orthographic volume rendering from any direction. A Python loop over the samples n, numpy
over the W x H image, every value in the dtype of the density, every expression bracketed as written. The sample is
stable_ref._Sample (§6), the opacity render_ref.opacity (§12). Fields are (N+2)^3, indexed [k, j, i]; images are
(height, width), indexed [b, a].

A frame is the tuple (origin, du, dv, step, samples, sigma, width, height): four double vectors ordered (x, y, z) =
(i, j, k), converted to T once. view_frame is the camera of §13 in double. render_view_slabs is the decomposition spelt
out: every slab applies the samples whose k0 it owns and hands the pair on; with the pair handed on intact it is
render_view operation for operation. The keyword arguments of `render_view` that default to the SPEC's rule exist so
that a rule that is NOT the SPEC's (tests/test_render_view_ref.py) has something to be told from."""
from collections import namedtuple

import numpy as np

import render_ref as RR
import stable_ref as S3

Frame = namedtuple("Frame", "origin du dv step samples sigma width height")


def _len(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def view_frame(N, direction, up, width, height, step, sigma):
    """The convenience camera of §13: all double, + - * / sqrt only, bracketed as written."""
    d = np.array(direction, np.float64)
    up = np.array(up, np.float64)
    d = d / _len(d)
    r = _cross(d, up)
    r = r / _len(r)
    u = _cross(r, d)
    L = np.sqrt(3.0) * N
    pix = L / max(width, height)
    c = (N + 1) / 2.0
    du, dv, ds = r * pix, u * pix, d * step
    origin = ((c - d * (L / 2)) - du * ((width - 1) / 2.0)) - dv * ((height - 1) / 2.0)
    return Frame(origin, du, dv, ds, int(L / step) + 1, sigma * step, width, height)


def axis_frame(N, axis, from_high, sigma):
    """The frame whose samples are the cell centres of render_ref's view (axis, from_high): exact in every dtype."""
    a_ax, b_ax = [x for x in range(3) if x != axis]
    du, dv, ds, o = np.zeros(3), np.zeros(3), np.zeros(3), np.ones(3)
    du[a_ax], dv[b_ax] = 1.0, 1.0
    ds[axis] = -1.0 if from_high else 1.0
    o[axis] = N if from_high else 1
    return Frame(o, du, dv, ds, N, sigma, N, N)


def position(fr, T, n):
    """The three (H, W) arrays of sample n: ((o + T(a) du) + T(b) dv) + T(n) ds, from n afresh."""
    a = np.arange(fr.width).astype(T)[None, :]
    b = np.arange(fr.height).astype(T)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        return [(((T(fr.origin[c]) + a * T(fr.du[c])) + b * T(fr.dv[c])) + T(n) * T(fr.step[c])).astype(T) for c in range(3)]


def visited(N, T, p, half_open=False):
    lo, hi = T(0.5), T(N) + T(0.5)
    with np.errstate(invalid="ignore"):
        v = np.ones(p[0].shape, bool)
        for x in p:
            v &= (x >= lo) & ((x < hi) if half_open else (x <= hi))
    return v


def owner_k(z, vis):
    """k0 of a visited sample with k0 = 0 counted as 1 (§6.1: it belongs to slab 0)."""
    k0 = np.where(vis, z, 1).astype(np.int64)
    return np.where(k0 == 0, 1, k0)


def start(fr, dtype):
    return np.zeros((fr.height, fr.width), dtype), np.ones((fr.height, fr.width), dtype)


def render_view(dens, emit, fr, krange=None, state=None, position=position, visited=visited, order=None,
                clamp_unvisited=False, nearest_emit=False, tr_first=False, owner=owner_k):
    """(C, Tr) after the samples of `order` (default 0 .. samples - 1) whose owner plane lies in krange (default: all)
    have been applied to `state` (default (+0, 1))."""
    N = dens.shape[0] - 2
    T = dens.dtype.type
    s = RR.scalar(N, dens.dtype, fr.sigma)
    C, Tr = start(fr, dens.dtype) if state is None else (state[0].copy(), state[1].copy())
    with np.errstate(invalid="ignore", over="ignore"):
        for n in (range(fr.samples) if order is None else order):
            p = position(fr, T, n)
            vis = visited(N, T, p)
            on = np.ones_like(vis) if clamp_unvisited else vis
            if krange is not None:
                ko = owner(p[2], vis)
                on = on & (ko >= krange[0]) & (ko <= krange[1])
            if not on.any():
                continue
            pos = np.stack([np.where(on, x, T(1)).ravel() for x in p], 1).astype(T)
            smp = S3._Sample(N, pos, S3.SPEC)
            a = RR.opacity(s, smp(dens).reshape(on.shape).astype(T))
            if emit is None:
                e = None
            elif nearest_emit:
                idx = [np.clip(np.floor(np.where(on, x, T(1)) + T(0.5)).astype(np.int64), 0, N + 1) for x in p]
                e = emit[idx[2], idx[1], idx[0]]
            else:
                e = smp(emit).reshape(on.shape).astype(T)
            if tr_first:
                Trn = Tr * (T(1) - a)
                Cn = C + (Trn * a) * e if e is not None else C + Trn * a
            else:
                Cn = C + (Tr * a) * e if e is not None else C + Tr * a
                Trn = Tr * (T(1) - a)
            C, Tr = np.where(on, Cn, C).astype(T), np.where(on, Trn, Tr).astype(T)
    return C, Tr


def chain_high(fr, dtype):
    """The slabs are visited downwards iff T(step_z) < 0."""
    T = np.dtype(dtype).type
    return bool(T(fr.step[2]) < T(0))


def render_view_slabs(dens, emit, fr, P, hand_on=lambda state, dtype: state, high=None, **kw):
    """The chain of §13 over P slabs of N / P planes; hand_on(state, dtype) is what crosses a slab boundary."""
    N = dens.shape[0] - 2
    nzl = N // P
    high = chain_high(fr, dens.dtype) if high is None else high
    state = start(fr, dens.dtype)
    for n, g in enumerate(range(P - 1, -1, -1) if high else range(P)):
        if n:
            state = hand_on(state, dens.dtype)
        state = render_view(dens, emit, fr, krange=(g * nzl + 1, (g + 1) * nzl), state=state, **kw)
    return state


def held_pixels(dens, emit, fr, P, rank):
    """What the context that holds the slabs `rank` of P reads back: the whole image where the last slab visited is
    among them, zeros elsewhere."""
    C, Tr = render_view(dens, emit, fr)
    last = 0 if chain_high(fr, dens.dtype) else P - 1
    if last in rank:
        return C, Tr
    return np.zeros_like(C), np.zeros_like(Tr)


def visit_counts(N, dtype, fr):
    """Per pixel, the number of samples visited."""
    T = np.dtype(dtype).type
    cnt = np.zeros((fr.height, fr.width), np.int64)
    for n in range(fr.samples):
        cnt += visited(N, T, position(fr, T, n))
    return cnt
