"""docs/SPEC.md §14 in numpy: perspective volume rendering, on top of tests/render_view_ref.py (§13). A Python loop over
the samples n, numpy over the W x H image, every value in the dtype of the density, every expression bracketed as
written. Fields are (N+2)^3, indexed [k, j, i]; images are (height, width), indexed [b, a].

A frame is a §13 frame (the first eight members, so that every helper of render_view_ref takes it) plus step_du and
step_dv: per pixel r = (step + T(a) step_du) + T(b) step_dv, sample n at base + T(n) r, and sigma the extinction per
cell length, scaled per pixel by |r|. camera_frame is the pinhole camera of §14 in double. render_camera_slabs is the
decomposition spelt out: the corner rule names the passes; a mixed frame takes an upward pass over the slabs that
applies the up pixels and then a downward pass, from the pair the upward pass left, that applies the down pixels. The
keyword arguments that default to the SPEC's rule exist so that a rule that is NOT the SPEC's
(tests/test_render_camera_ref.py) has something to be told from."""
from collections import namedtuple

import numpy as np

import render_ref as RR
import render_view_ref as VR
import stable_ref as S3

Frame = namedtuple("Frame", "origin du dv step samples sigma width height step_du step_dv")
UP, DOWN, BOTH = 0, 1, 2  # sf_camera_passes


def of_view(fr, sigma=None):
    """The §13 frame as a camera frame: step_du = step_dv = 0. sigma: per cell length (default: the view's, which for a
    step vector of length 1 is the same thing)."""
    return Frame(*fr[:5], fr.sigma if sigma is None else sigma, fr.width, fr.height, np.zeros(3), np.zeros(3))


def camera_frame(N, eye, target, up, tan_half_fov, width, height, step, sigma):
    """The pinhole camera of §14: all double, + - * / sqrt only, bracketed as written. None where the SPEC refuses."""
    eye, target, up = (np.array(v, np.float64) for v in (eye, target, up))
    f = target - eye
    lf = VR._len(f)
    if not (lf > 0.0 and tan_half_fov > 0.0 and step > 0.0):
        return None
    d = f / lf
    r = VR._cross(d, up)
    lr = VR._len(r)
    if not lr > 0.0:
        return None
    r = r / lr
    u = VR._cross(r, d)
    R = np.sqrt(3.0) * N / 2.0
    c = (N + 1) / 2.0
    e = c - eye
    dc = (e[0] * d[0] + e[1] * d[1]) + e[2] * d[2]
    t0 = dc - R
    if not t0 > 0:
        t0 = 0.0
    t1 = dc + R
    if not t1 > t0 or not (t1 - t0) / step < 65536.0:
        return None
    pp = (2.0 * tan_half_fov) / height
    q0 = (d - r * (pp * ((width - 1) / 2.0))) - u * (pp * ((height - 1) / 2.0))
    return Frame(eye + q0 * t0, r * (pp * t0), u * (pp * t0), q0 * step, int((t1 - t0) / step) + 1, sigma, width, height,
                 r * (pp * step), u * (pp * step))


def _ab(fr, T):
    return np.arange(fr.width).astype(T)[None, :], np.arange(fr.height).astype(T)[:, None]


def direction(fr, T):
    """The three (H, W) arrays of r = (ds + T(a) dsu) + T(b) dsv."""
    a, b = _ab(fr, T)
    with np.errstate(invalid="ignore", over="ignore"):
        return [((T(fr.step[c]) + a * T(fr.step_du[c])) + b * T(fr.step_dv[c])).astype(T) for c in range(3)]


def position(fr, T, n, direction=direction):
    """The three (H, W) arrays of sample n: ((o + T(a) du) + T(b) dv) + T(n) r, from n afresh."""
    a, b = _ab(fr, T)
    r = direction(fr, T)
    with np.errstate(invalid="ignore", over="ignore"):
        return [(((T(fr.origin[c]) + a * T(fr.du[c])) + b * T(fr.dv[c])) + T(n) * r[c]).astype(T) for c in range(3)]


def length(r):
    return np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])


def scalar(fr, N, T, r, length=length):
    """s_ab = (T(sigma) * h) * |r|, an (H, W) array."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (RR.scalar(N, T, fr.sigma) * length(r).astype(T)).astype(T)


def is_down(fr, T, direction=direction):
    """The (H, W) mask of the down pixels: r_z < T(0)."""
    with np.errstate(invalid="ignore"):
        return direction(fr, T)[2] < T(0)


def render_camera(dens, emit, fr, krange=None, state=None, only=None, position=position, direction=direction,
                  scalar=scalar):
    """(C, Tr) after the samples 0 .. samples - 1 of the pixels of the mask `only` (default: all) whose owner plane lies
    in krange (default: all) have been applied to `state` (default (+0, 1))."""
    N = dens.shape[0] - 2
    T = dens.dtype.type
    s = scalar(fr, N, T, direction(fr, T))
    C, Tr = VR.start(fr, dens.dtype) if state is None else (state[0].copy(), state[1].copy())
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(fr.samples):
            p = position(fr, T, n, direction)
            on = VR.visited(N, T, p)
            if only is not None:
                on = on & only
            if krange is not None:
                ko = VR.owner_k(p[2], on)
                on = on & (ko >= krange[0]) & (ko <= krange[1])
            if not on.any():
                continue
            pos = np.stack([np.where(on, x, T(1)).ravel() for x in p], 1).astype(T)
            smp = S3._Sample(N, pos, S3.SPEC)
            a = RR.opacity(s, smp(dens).reshape(on.shape).astype(T))
            if emit is None:
                Cn = C + Tr * a
            else:
                Cn = C + (Tr * a) * smp(emit).reshape(on.shape).astype(T)
            Trn = Tr * (T(1) - a)
            C, Tr = np.where(on, Cn, C).astype(T), np.where(on, Trn, Tr).astype(T)
    return C, Tr


def corner_rule(fr, T, direction=direction):
    down = is_down(fr, T, direction)
    corners = [bool(down[b, a]) for a in (0, -1) for b in (0, -1)]
    return DOWN if all(corners) else (BOTH if any(corners) else UP)


def passes(fr, dtype, rule=corner_rule):
    """UP, DOWN or BOTH: the corner rule of §14 in T."""
    return rule(fr, np.dtype(dtype).type)


def render_camera_slabs(dens, emit, fr, P, rule=corner_rule, restart_down=False, mask_down=True, down_of=is_down,
                        single_up=False, **kw):
    """The chain of §14 over P slabs of N / P planes, the whole pair handed on in both passes."""
    N = dens.shape[0] - 2
    T = dens.dtype.type
    nzl = N // P
    what = UP if single_up else rule(fr, T)
    down = down_of(fr, T)
    state = VR.start(fr, dens.dtype)
    if P == 1:
        return render_camera(dens, emit, fr, krange=(1, N), state=state, **kw)
    if what in (UP, BOTH):
        for g in range(P):
            state = render_camera(dens, emit, fr, krange=(g * nzl + 1, (g + 1) * nzl), state=state,
                                  only=~down if what == BOTH else None, **kw)
    if what in (DOWN, BOTH):
        if restart_down:
            state = VR.start(fr, dens.dtype)
        for g in range(P - 1, -1, -1):
            state = render_camera(dens, emit, fr, krange=(g * nzl + 1, (g + 1) * nzl), state=state,
                                  only=down if (what == BOTH and mask_down) else None, **kw)
    return state


def last_slab(fr, dtype, P, rule=corner_rule, mixed_ends_on_top=False):
    """The slab the image ends on: the last one visited."""
    what = passes(fr, dtype, rule)
    return P - 1 if what == UP or (what == BOTH and mixed_ends_on_top) else 0


def held_pixels(dens, emit, fr, P, rank, **kw):
    """What the context that holds the slabs `rank` of P reads back: the whole image where the last slab visited is
    among them, zeros elsewhere."""
    C, Tr = render_camera(dens, emit, fr)
    if last_slab(fr, dens.dtype, P, **kw) in rank:
        return C, Tr
    return np.zeros_like(C), np.zeros_like(Tr)


def visit_counts(N, dtype, fr):
    """Per pixel, the number of samples visited."""
    T = np.dtype(dtype).type
    cnt = np.zeros((fr.height, fr.width), np.int64)
    for n in range(fr.samples):
        cnt += VR.visited(N, T, position(fr, T, n))
    return cnt


def slabs_crossed(N, dtype, fr, P):
    """Per pixel, the number of slabs (of P) that own a visited sample of it."""
    T = np.dtype(dtype).type
    nzl = N // P
    seen = np.zeros((P, fr.height, fr.width), bool)
    for n in range(fr.samples):
        p = position(fr, T, n)
        vis = VR.visited(N, T, p)
        g = (VR.owner_k(p[2], vis) - 1) // nzl
        for s in range(P):
            seen[s] |= vis & (g == s)
    return seen.sum(0)
