"""CPU reference of docs/SPEC.md §9 (limited MacCormack advection) in numpy, built on the CPU oracle's `advect`.

Arrays are (N+2,)*3 indexed [k, j, i], in the context's dtype (float32 / float64). `hat` is `oracle_lib.advect`, `bar`
is `oracle_lib.advect` of `hat` with `-dt` (the same bits as the SPEC's reverse trace: `(-dt)*Nf` is `-(dt*Nf)` exactly
and `i - (-a)` is `i + a`); only bar's interior is used. The trace indices, the clamp flags and the min / max selects
are numpy operations on the dtype, one rounding each, in the SPEC's bracketing. set_bnd is the oracle's.
`step(...)` is vel_step + dens_step of SPEC §3 composed from the oracle's public operators, `advect_mc` in place of
`advect` where a scheme is on (and the §8 forces of tests/forces_ref.py in front when given)."""
import numpy as np

import forces_ref as F
import oracle_lib as O

SEMI_LAGRANGIAN, MACCORMACK = 0, 1
I = (slice(1, -1),) * 3


def sel_min(p, q):
    return np.where(q < p, q, p)


def sel_max(p, q):
    return np.where(q > p, q, p)


def trace_positions(vel, dt0, sign):
    """One trace of every interior cell: ((i0, j0, k0), clamped, (x, y, z)) with the clamped positions the weights are
    taken from. sign = -1: x = i - dt0*u (forward trace of §3), +1: x = i + dt0*u (reverse trace). Indices as §3:
    (int)x, NaN -> 0, clamped into [0, N]."""
    T = vel[0].dtype.type
    N = vel[0].shape[0] - 2
    lo, hi = T(0.5), T(N) + T(0.5)
    idx = np.arange(1, N + 1).astype(T)
    clamped = np.zeros((N, N, N), bool)
    out, pos = [], []
    with np.errstate(invalid="ignore"):
        for ax, comp in enumerate(vel):  # ax 0: i (last array axis)
            shape = [1, 1, 1]
            shape[2 - ax] = N
            a = dt0 * comp[I]
            x = idx.reshape(shape) - a if sign < 0 else idx.reshape(shape) + a
            clamped |= (x < lo) | (x > hi)
            x = np.where(x < lo, lo, x)
            x = np.where(x > hi, hi, x)
            i0 = np.where(x == x, x, T(0)).astype(np.int64)
            out.append(np.clip(i0, 0, N))
            pos.append(x)
    return out, clamped, pos


def trace(vel, dt0, sign):
    """((i0, j0, k0), clamped) of trace_positions."""
    idx, clamped, _ = trace_positions(vel, dt0, sign)
    return idx, clamped


def next_cell_adjacent(idx):
    """(N, N, N-1) bools [k-1, j-1, i-1], i = 1..N-1: the (i0, j0, k0) of cell i+1 is (i0+1, j0, k0) of cell i — the
    condition under which a one-cell-per-lane kernel may take cell i's i0+1 samples from the lane of cell i+1."""
    i0, j0, k0 = idx
    return ((i0[:, :, 1:] == i0[:, :, :-1] + 1) & (j0[:, :, 1:] == j0[:, :, :-1]) & (k0[:, :, 1:] == k0[:, :, :-1]))


def adjacency(u, v, w, dt, lanes=64):
    """Fractions (forward, reverse) of the cells with a next lane in their wave (i < N, (i-1) % lanes != lanes-1) whose
    next cell's trace is adjacent in the sense of next_cell_adjacent."""
    T = u.dtype.type
    N = u.shape[0] - 2
    dt0 = T(dt) * T(N)
    has_next = (np.arange(N - 1) % lanes) != lanes - 1
    out = []
    for sign in (-1, +1):
        idx, _ = trace((u, v, w), dt0, sign)
        adj = next_cell_adjacent(idx)[:, :, has_next]
        out.append(float(adj.mean()) if adj.size else 0.0)
    return tuple(out)


def parts(b, d0, u, v, w, dt):
    """Everything SPEC §9 step 2 names, on the interior cells: dict with hat (whole field), bar, mn, mx, raw (the
    unlimited value), cf, cr."""
    T = d0.dtype.type
    N = d0.shape[0] - 2
    dt = T(dt)
    dt0 = dt * T(N)
    hat = np.zeros_like(d0)
    O.advect(b, hat, d0, u, v, w, dt)
    bar = np.zeros_like(d0)
    O.advect(0, bar, hat, u, v, w, -dt)
    (i0, j0, k0), cf = trace((u, v, w), dt0, -1)
    _, cr = trace((u, v, w), dt0, +1)

    def a(x, y, z):
        return d0[k0 + z, j0 + y, i0 + x]

    mn = sel_min(sel_min(sel_min(a(0, 0, 0), a(0, 0, 1)), sel_min(a(0, 1, 0), a(0, 1, 1))),
                 sel_min(sel_min(a(1, 0, 0), a(1, 0, 1)), sel_min(a(1, 1, 0), a(1, 1, 1))))
    mx = sel_max(sel_max(sel_max(a(0, 0, 0), a(0, 0, 1)), sel_max(a(0, 1, 0), a(0, 1, 1))),
                 sel_max(sel_max(a(1, 0, 0), a(1, 0, 1)), sel_max(a(1, 1, 0), a(1, 1, 1))))
    with np.errstate(invalid="ignore"):
        raw = hat[I] + T(0.5) * (d0[I] - bar[I])
    return {"hat": hat, "bar": bar[I], "mn": mn, "mx": mx, "raw": raw, "cf": cf, "cr": cr}


def advect_mc(b, d, d0, u, v, w, dt):
    """SPEC §9 advect_mc; d is written in place (every entry) and returned."""
    p = parts(b, d0, u, v, w, dt)
    with np.errstate(invalid="ignore"):
        r = p["raw"]
        r = np.where(r < p["mn"], p["mn"], r)
        r = np.where(r > p["mx"], p["mx"], r)
        r = np.where(p["cf"] | p["cr"], p["hat"][I], r)
    d[...] = 0
    d[I] = r
    O.set_bnd(b, d)
    return d


def outcomes(d0, u, v, w, dt):
    """Fractions of the interior cells that take each outcome: (fallback, limited, unlimited)."""
    p = parts(0, d0, u, v, w, dt)
    fb = p["cf"] | p["cr"]
    lim = ~fb & ((p["raw"] < p["mn"]) | (p["raw"] > p["mx"]))
    return float(fb.mean()), float(lim.mean()), float((~fb & ~lim).mean())


def _advect(scheme):
    return advect_mc if scheme == MACCORMACK else O.advect


def vel_step(u, v, w, u0, v0, w0, visc, dt, K, scheme=SEMI_LAGRANGIAN):
    """SPEC §3 vel_step, operator by operator, with the velocity scheme given. In place: on return the arrays hold what
    their names hold after the oracle's vel_step."""
    adv = _advect(scheme)
    for x, s in ((u, u0), (v, v0), (w, w0)):
        O.add_source(x, s, dt)
    u, u0, v, v0, w, w0 = u0, u, v0, v, w0, w
    O.diffuse(1, u, u0, visc, dt, K)
    O.diffuse(2, v, v0, visc, dt, K)
    O.diffuse(3, w, w0, visc, dt, K)
    O.project(u, v, w, u0, v0, K)
    u, u0, v, v0, w, w0 = u0, u, v0, v, w0, w
    adv(1, u, u0, u0, v0, w0, dt)
    adv(2, v, v0, u0, v0, w0, dt)
    adv(3, w, w0, u0, v0, w0, dt)
    O.project(u, v, w, u0, v0, K)


def dens_step(x, x0, u, v, w, diff, dt, K, scheme=SEMI_LAGRANGIAN):
    """SPEC §3 dens_step with the density scheme given; in place."""
    O.add_source(x, x0, dt)
    x, x0 = x0, x
    O.diffuse(0, x, x0, diff, dt, K)
    x, x0 = x0, x
    _advect(scheme)(0, x, x0, u, v, w, dt)


def step(fields, dt, diff, visc, K, velocity=SEMI_LAGRANGIAN, density=SEMI_LAGRANGIAN, bound=None, eps=0.0,
         beta=0.0, ambient=0.0, axis=1):
    """vel_step then dens_step on a dict of the 8 named fields (in place; returned) with the schemes given. `bound`:
    {"u0": array, ...} bound sources, copied into the x0 slots first (sf_bind_sources). eps / beta: the §8 forces."""
    f = fields
    T = f["u"].dtype.type
    if bound:
        for n, a in bound.items():
            f[n][...] = a
    F.add_forces(f["u"], f["v"], f["w"], f["dens"], f["u0"], f["v0"], f["w0"], eps, beta, ambient, axis)
    vel_step(f["u"], f["v"], f["w"], f["u0"], f["v0"], f["w0"], T(visc), T(dt), K, velocity)
    dens_step(f["dens"], f["dens0"], f["u"], f["v"], f["w"], T(diff), T(dt), K, density)
    return f
