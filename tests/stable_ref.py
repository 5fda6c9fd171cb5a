"""docs/SPEC.md §3 and §6 in numpy: add_source, set_bnd, lin_solve, advect, project_div, project_sub, project,
tracers_advect, tracers_sample. A second statement of the text next to the C++ oracle, so that the two pin each other
in bits (tests/test_stable_inputs_ref.py) and so that a plausible kernel error can be written into a copy of it.

Arrays are (N+2,)*3 indexed [k, j, i] in float32 / float64 and modified in place, as in tests/oracle_lib.py. Every
scalar is a T, every expression bracketed as in the SPEC, one rounding per operation. Clamps are the SPEC's compares
(np.where): np.minimum / np.maximum / np.clip on floats, which treat a NaN their own way, occur nowhere. The
back-trace is maccormack_ref.trace_positions.

The expressions that a kernel could form another way sit in the methods of `Ops`; every operator takes `ops`, the
SPEC's by default. The mutants of tests/test_stable_inputs_ref.py are subclasses of Ops in that file."""
import numpy as np

import maccormack_ref as M

I = (slice(1, -1),) * 3


def where_clamp(x, lo, hi):
    """if (x < lo) x = lo; if (x > hi) x = hi: a NaN stays."""
    with np.errstate(invalid="ignore"):
        x = np.where(x < lo, lo, x)
        return np.where(x > hi, hi, x)


class Ops:
    def face(self, s, v):
        """A face cell of set_bnd: s * v with s = -1 or 1."""
        return s * v

    def edge(self, half, a, b):
        return half * (a + b)

    def sweep(self, x, x0, a, inv, it):
        """The interior of one Jacobi sweep (it: its number in the solve, 0 first)."""
        with np.errstate(invalid="ignore", over="ignore"):
            return (x0[I] + a * (((x[1:-1, 1:-1, :-2] + x[1:-1, 1:-1, 2:]) + (x[1:-1, :-2, 1:-1] + x[1:-1, 2:, 1:-1]))
                                 + (x[:-2, 1:-1, 1:-1] + x[2:, 1:-1, 1:-1]))) * inv

    def trace(self, vel, dt0):
        """((i0, j0, k0), (x, y, z)) of every interior cell."""
        idx, _, pos = M.trace_positions(vel, dt0, -1)
        return idx, pos

    def combine(self, s0, lo, s1, hi):
        """s0 * (the four i0 samples, combined) + s1 * (the four i0 + 1 samples, combined)."""
        return s0 * lo + s1 * hi

    def grad_sub(self, u, c_grad, pp, pm):
        return u - c_grad * (pp - pm)

    def clamp_coord(self, x, lo, hi):
        """The clamp of a tracer coordinate (SPEC §6)."""
        return where_clamp(x, lo, hi)

    # the masked operators (SPEC §15 to §17: obstacles_ref, obstacles_mg_ref, obstacle_transport_ref) state their own
    # stencils; what they share with the methods above is trace, combine and these two
    def neg(self, x):
        """effn: the cell's own value as the operand across a closed face on the field's own axis."""
        return -x

    def sweep_io(self, x):
        """A field as a masked sweep loads it, and the values the sweep stores."""
        return x


SPEC = Ops()


def add_source(x, s, dt):
    with np.errstate(invalid="ignore", over="ignore"):
        x[...] = x + x.dtype.type(dt) * s


def set_bnd(b, x, ops=SPEC):
    T = x.dtype.type
    sx, sy, sz = (T(-1) if b == ax else T(1) for ax in (1, 2, 3))
    half, third = T(0.5), T(1.0 / 3.0)
    m = slice(1, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo, inn in ((0, 1), (-1, -2)):
            x[m, m, lo] = ops.face(sx, x[m, m, inn])
        for lo, inn in ((0, 1), (-1, -2)):
            x[m, lo, m] = ops.face(sy, x[m, inn, m])
        for lo, inn in ((0, 1), (-1, -2)):
            x[lo, m, m] = ops.face(sz, x[inn, m, m])
        ends = ((0, 1), (-1, -2))
        for J, Jn in ends:  # x-directed: x[i, J, K] = half * (x[i, Jn, K] + x[i, J, Kn])
            for K, Kn in ends:
                x[K, J, m] = ops.edge(half, x[K, Jn, m], x[Kn, J, m])
        for I_, In in ends:  # y-directed: x[I, j, K] = half * (x[In, j, K] + x[I, j, Kn])
            for K, Kn in ends:
                x[K, m, I_] = ops.edge(half, x[K, m, In], x[Kn, m, I_])
        for I_, In in ends:  # z-directed: x[I, J, k] = half * (x[In, J, k] + x[I, Jn, k])
            for J, Jn in ends:
                x[m, J, I_] = ops.edge(half, x[m, J, In], x[m, Jn, I_])
        for I_, In in ends:
            for J, Jn in ends:
                for K, Kn in ends:
                    x[K, J, I_] = third * ((x[K, J, In] + x[K, Jn, I_]) + x[Kn, J, I_])


def lin_solve(b, x, x0, a, c, K, ops=SPEC):
    T = x.dtype.type
    a, inv = T(a), T(1) / T(c)
    cur = x.copy()
    for it in range(K):
        nxt = np.zeros_like(cur)  # (a sweep and its set_bnd write every entry)
        nxt[I] = ops.sweep(cur, x0, a, inv, it)
        set_bnd(b, nxt, ops)
        cur = nxt
    x[...] = cur


def advect(b, d, d0, u, v, w, dt, ops=SPEC):
    T = d.dtype.type
    N = d.shape[0] - 2
    dt0 = T(dt) * T(N)
    (i0, j0, k0), (x, y, z) = ops.trace((u, v, w), dt0)
    with np.errstate(invalid="ignore", over="ignore"):
        s1, t1, r1 = x - i0.astype(T), y - j0.astype(T), z - k0.astype(T)
        s0, t0, r0 = T(1) - s1, T(1) - t1, T(1) - r1

        def at(di, dj, dk):
            return d0[k0 + dk, j0 + dj, i0 + di]

        def plane(di):
            return (t0 * (r0 * at(di, 0, 0) + r1 * at(di, 0, 1)) + t1 * (r0 * at(di, 1, 0) + r1 * at(di, 1, 1)))

        d[I] = ops.combine(s0, plane(0), s1, plane(1))
    set_bnd(b, d, ops)


def project_div(u, v, w, p, div, ops=SPEC):
    T = u.dtype.type
    N = u.shape[0] - 2
    c_div = T(-0.5) * (T(1) / T(N))
    p[...] = T(0)
    with np.errstate(invalid="ignore", over="ignore"):
        div[I] = c_div * (((u[1:-1, 1:-1, 2:] - u[1:-1, 1:-1, :-2]) + (v[1:-1, 2:, 1:-1] - v[1:-1, :-2, 1:-1]))
                          + (w[2:, 1:-1, 1:-1] - w[:-2, 1:-1, 1:-1]))
    set_bnd(0, div, ops)
    set_bnd(0, p, ops)


def project_sub(u, v, w, p, ops=SPEC):
    T = u.dtype.type
    c_grad = T(0.5) * T(u.shape[0] - 2)
    with np.errstate(invalid="ignore", over="ignore"):
        u[I] = ops.grad_sub(u[I], c_grad, p[1:-1, 1:-1, 2:], p[1:-1, 1:-1, :-2])
        v[I] = ops.grad_sub(v[I], c_grad, p[1:-1, 2:, 1:-1], p[1:-1, :-2, 1:-1])
        w[I] = ops.grad_sub(w[I], c_grad, p[2:, 1:-1, 1:-1], p[:-2, 1:-1, 1:-1])
    set_bnd(1, u, ops)
    set_bnd(2, v, ops)
    set_bnd(3, w, ops)


def project(u, v, w, p, div, K, ops=SPEC):
    project_div(u, v, w, p, div, ops)
    lin_solve(0, p, div, 1, 6, K, ops)
    project_sub(u, v, w, p, ops)


class _Sample:
    """The trilinear sample of SPEC §6 at positions (n, 3): clamp, (int)x with NaN -> 0 clamped into [0, N], weights."""

    def __init__(self, N, pos, ops):
        T = pos.dtype.type
        lo, hi = T(0.5), T(N) + T(0.5)
        self.q, self.wt = [], []
        with np.errstate(invalid="ignore"):
            for ax in range(3):
                x = ops.clamp_coord(pos[:, ax], lo, hi)
                i0 = np.where(x == x, x, T(0)).astype(np.int64)
                i0 = np.where(i0 < 0, 0, np.where(i0 > N, N, i0))
                s1 = x - i0.astype(T)
                self.q.append(i0)
                self.wt.append((T(1) - s1, s1))

    def __call__(self, f):
        (i0, j0, k0), ((s0, s1), (t0, t1), (r0, r1)) = self.q, self.wt

        def at(di, dj, dk):
            return f[k0 + dk, j0 + dj, i0 + di]

        with np.errstate(invalid="ignore", over="ignore"):
            return (s0 * (t0 * (r0 * at(0, 0, 0) + r1 * at(0, 0, 1)) + t1 * (r0 * at(0, 1, 0) + r1 * at(0, 1, 1)))
                    + s1 * (t0 * (r0 * at(1, 0, 0) + r1 * at(1, 0, 1)) + t1 * (r0 * at(1, 1, 0) + r1 * at(1, 1, 1))))


def tracers_advect(pos, u, v, w, dt, ops=SPEC):
    T = pos.dtype.type
    N = u.shape[0] - 2
    dt0, lo, hi = T(dt) * T(N), T(0.5), T(N) + T(0.5)
    p = np.stack([ops.clamp_coord(pos[:, ax], lo, hi) for ax in range(3)], axis=1)
    s = _Sample(N, p, ops)
    with np.errstate(invalid="ignore", over="ignore"):
        for ax, f in enumerate((u, v, w)):
            pos[:, ax] = ops.clamp_coord(p[:, ax] + dt0 * s(f), lo, hi)


def tracers_sample(pos, dens, u, v, w, ops=SPEC):
    s = _Sample(u.shape[0] - 2, pos, ops)
    a, b, c = s(u), s(v), s(w)
    with np.errstate(invalid="ignore", over="ignore"):
        return s(dens), np.sqrt((a * a + b * b) + c * c)
