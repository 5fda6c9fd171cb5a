"""numpy reference of docs/SPEC.md §18 "MacCormack under the mask", written from the SPEC text on
tests/obstacle_transport_ref.py (advect_masked), tests/maccormack_ref.py (trace_positions, sel_min, sel_max),
tests/obstacles_ref.py (Mask, solid_cells) and tests/stable_ref.py (set_bnd). It does not call the library. Fields and
the mask are (N+2, N+2, N+2) arrays indexed [k, j, i]; every per-cell expression is one numpy operation per SPEC operation
on the dtype, every rule a select (np.where) on values that are all evaluated.

`wrong` names one deliberately wrong reading of §18 (WRONG): tests/test_obstacle_maccormack_ref.py shows for each of them
a case whose result it changes, so that a test against this reference tells that reading from the SPEC's. `slabs`
emulates the k-slabs of a decomposed context for the two readings that leave a ghost plane stale.
"""
import numpy as np

import maccormack_ref as MR
import obstacle_transport_ref as TR
import obstacles_ref as OB
import stable_ref as S3

I = TR.I
SEMI_LAGRANGIAN, MACCORMACK = MR.SEMI_LAGRANGIAN, MR.MACCORMACK
WRONG = ("pass1_unmasked", "no_solid_fallback", "sf_only", "sr_only", "sr_at_forward", "solidity_of_i0_reverse",
         "solids_not_zeroed", "hat_ghost_stale", "code_ghost_stale_reverse", "hw_minmax")
CORNERS = [(di, dj, dk) for di in (0, 1) for dj in (0, 1) for dk in (0, 1)]


def parts(b, d0, u, v, w, dt, mask, wrong=None, slabs=1):
    """Everything §18 names, on the interior cells: dict with hat (the whole field), bar, mn, mx, raw (the unlimited
    value), cf, cr, sf, sr, solid, fluid."""
    T = d0.dtype.type
    N = d0.shape[0] - 2
    mk = OB.Mask(mask)
    solid = OB.solid_cells(mask)  # (N+2)^3: a sample in the shell is never solid
    dt0 = T(dt) * T(N)
    hat = np.zeros_like(d0)
    if wrong == "pass1_unmasked":
        S3.advect(b, hat, d0, u, v, w, dt)
    else:
        TR.advect_masked(b, hat, d0, u, v, w, dt, mask)
    (fi, fj, fk), cf, _ = MR.trace_positions((u, v, w), dt0, -1)
    (ri, rj, rk), cr, (x, y, z) = MR.trace_positions((u, v, w), dt0, +1)
    kc = np.arange(1, N + 1).reshape(N, 1, 1)
    nzl = N // slabs

    def across(ks):  # the sample plane belongs to another slab than the cell's
        return (ks >= 1) & (ks <= N) & ((ks - 1) // nzl != (kc - 1) // nzl)

    def a(di, dj, dk):
        return d0[fk + dk, fj + dj, fi + di]

    def h(di, dj, dk):
        val = hat[rk + dk, rj + dj, ri + di]
        if wrong == "hat_ghost_stale":  # the ghost planes still hold what they held before pass 1: here +0
            val = np.where(across(rk + dk), T(0), val)
        return val

    sf = np.zeros((N,) * 3, bool)
    sr = np.zeros((N,) * 3, bool)
    for di, dj, dk in CORNERS:
        sf |= solid[fk + dk, fj + dj, fi + di]
        if wrong == "sr_at_forward":
            s = solid[fk + dk, fj + dj, fi + di]
        else:
            s = solid[rk + dk, rj + dj, ri + (0 if wrong == "solidity_of_i0_reverse" else di)]
            if wrong == "code_ghost_stale_reverse":  # the code across a slab boundary reads as fluid
                s = s & ~across(rk + dk)
        sr |= s
    lo, hi = (np.fmin, np.fmax) if wrong == "hw_minmax" else (MR.sel_min, MR.sel_max)
    with np.errstate(invalid="ignore", over="ignore"):
        mn = lo(lo(lo(a(0, 0, 0), a(0, 0, 1)), lo(a(0, 1, 0), a(0, 1, 1))),
                lo(lo(a(1, 0, 0), a(1, 0, 1)), lo(a(1, 1, 0), a(1, 1, 1))))
        mx = hi(hi(hi(a(0, 0, 0), a(0, 0, 1)), hi(a(0, 1, 0), a(0, 1, 1))),
                hi(hi(a(1, 0, 0), a(1, 0, 1)), hi(a(1, 1, 0), a(1, 1, 1))))
        s1, t1, r1 = x - ri.astype(T), y - rj.astype(T), z - rk.astype(T)
        s0, t0, r0 = T(1) - s1, T(1) - t1, T(1) - r1

        def plane(di):
            return (t0 * (r0 * h(di, 0, 0) + r1 * h(di, 0, 1)) + t1 * (r0 * h(di, 1, 0) + r1 * h(di, 1, 1)))

        bar = s0 * plane(0) + s1 * plane(1)
        raw = hat[I] + T(0.5) * (d0[I] - bar)
    return {"hat": hat, "bar": bar, "mn": mn, "mx": mx, "raw": raw, "cf": cf, "cr": cr, "sf": sf, "sr": sr,
            "solid": mk.solid, "fluid": mk.fluid}


def fallback(p, wrong=None):
    fb = p["cf"] | p["cr"]
    if wrong == "no_solid_fallback":
        return fb
    if wrong == "sf_only":
        return fb | p["sf"]
    if wrong == "sr_only":
        return fb | p["sr"]
    return fb | p["sf"] | p["sr"]


def advect_mc_masked(b, d, d0, u, v, w, dt, mask, wrong=None, slabs=1):
    """§18 advect_mc_masked; d is written in place (every entry) and returned."""
    p = parts(b, d0, u, v, w, dt, mask, wrong, slabs)
    T = d.dtype.type
    with np.errstate(invalid="ignore"):
        r = p["raw"]
        r = np.where(r < p["mn"], p["mn"], r)
        r = np.where(r > p["mx"], p["mx"], r)
        r = np.where(fallback(p, wrong), p["hat"][I], r)
    if wrong != "solids_not_zeroed":
        r = np.where(p["solid"], T(0), r)
    d[...] = 0
    d[I] = r
    S3.set_bnd(b, d)
    return d


def outcomes(p):
    """Counts over the fluid cells: dict with fluid, second (no fallback), limited (second order and limited), sf_alone,
    sr_alone (the fallbacks only that flag raises)."""
    fl = p["fluid"]
    fb = fallback(p)
    with np.errstate(invalid="ignore"):
        lim = (p["raw"] < p["mn"]) | (p["raw"] > p["mx"])
    wall = p["cf"] | p["cr"]
    return {"fluid": int(fl.sum()), "second": int((fl & ~fb).sum()), "limited": int((fl & ~fb & lim).sum()),
            "sf_alone": int((fl & ~wall & p["sf"] & ~p["sr"]).sum()),
            "sr_alone": int((fl & ~wall & p["sr"] & ~p["sf"]).sum())}


def _advect(scheme, b, d, d0, u, v, w, dt, mask):
    if scheme == MACCORMACK:
        advect_mc_masked(b, d, d0, u, v, w, dt, mask)
    else:
        TR.advect_masked(b, d, d0, u, v, w, dt, mask)


def vel_step(f, mask, K, dt, visc, project, sources=None, forces=None, scheme=MACCORMACK):
    """obstacle_transport_ref.vel_step with the three advect_masked replaced by the velocity scheme's operator."""
    u, v, w, u0, v0, w0 = (f[n].copy() for n in ("u", "v", "w", "u0", "v0", "w0"))
    if sources:
        u0, v0, w0 = (sources[n].copy() for n in ("u0", "v0", "w0"))
    if forces:
        TR.F.add_forces(u, v, w, f["dens"], u0, v0, w0, **forces)
    for x, s in ((u, u0), (v, v0), (w, w0)):
        S3.add_source(x, s, dt)
    u, u0, v, v0, w, w0 = u0, u, v0, v, w0, w
    for b, x, x0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        TR.diffuse_masked(b, x, x0, visc, dt, K, mask)
    out = project(u, v, w)
    u0, v0, w0 = out["u"], out["v"], out["w"]
    u, v, w = (np.zeros_like(u0) for _ in range(3))
    for b, d, d0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        _advect(scheme, b, d, d0, u0, v0, w0, dt, mask)
    return project(u, v, w)


def dens_step(dens, dens0, u, v, w, mask, K, dt, diff, source=None, scheme=MACCORMACK):
    """obstacle_transport_ref.dens_step with the advect_masked replaced by the density scheme's operator."""
    x, x0 = dens.copy(), (source if source is not None else dens0).copy()
    S3.add_source(x, x0, dt)
    x, x0 = x0, x
    TR.diffuse_masked(0, x, x0, diff, dt, K, mask)
    x, x0 = x0, x
    _advect(scheme, 0, x, x0, u, v, w, dt, mask)
    return x
