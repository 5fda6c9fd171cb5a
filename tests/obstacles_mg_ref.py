"""numpy reference of docs/SPEC.md §16 "Obstacle-aware multigrid", written from the SPEC text on the pieces of
tests/obstacles_ref.py (Mask, the masked A, divergence, gradient), tests/pressure_mg_ref.py (levels, restrict) and
tests/pressure_cg_ref.py (set_bnd, the §10 sums). It does not call the library. Fields are (n+2)^3 arrays [k, j, i],
right-hand sides interior-shaped; one numpy operation per SPEC operation on the dtype, every solid and face rule a
select (np.where) on values that are all evaluated.

`wrong` names one deliberately wrong reading of §16 (WRONG); tests/test_obstacles_mg_ref.py shows for each a case of the
GPU file whose result it changes, or (EQUIVALENT) shows that no input can tell it from the SPEC's reading.
"""
import math

import numpy as np

import obstacles_ref as O
import pressure_cg_ref as R
import pressure_mg_ref as G
import stable_ref as S3

I = R.I
CONVERGED, MAX_ITERS, BREAKDOWN = R.CONVERGED, R.MAX_ITERS, R.BREAKDOWN
WRONG = ("coarse_ge4", "coarse_any", "coarse_unmasked", "solids_not_zeroed", "prolong_into_solids", "e_not_zeroed",
         "stale_code", "coarse_ghost_fluid")
# step 5's "+0 on solid cells" is followed by nu >= 1 masked sweeps, which write +0 there again and read no solid cell
EQUIVALENT = ("prolong_into_solids",)
# a wrong reading that only a right-hand side with -0 products tells from the SPEC's
# (tests/test_obstacle_special_inputs_ref.py)
SPECIAL_WRONG = ("first_smooth_no_zero",)


def coarsen(solid, wrong=None):
    """solid: interior-shaped bool (n, n, n), n even. The next level's: solid iff all eight children are solid."""
    lo, hi = slice(0, None, 2), slice(1, None, 2)
    count = sum(solid[k, j, i].astype(np.int64) for k in (lo, hi) for j in (lo, hi) for i in (lo, hi))
    return count >= {"coarse_ge4": 4, "coarse_any": 1}.get(wrong, 8)


def level_masks(mask, ns, wrong=None, slabs=1, stale_mask=None):
    """One obstacles_ref.Mask per level of sizes ns. Level 0 is §15's mask; the coarse levels come from coarsen().
    stale_mask (wrong "stale_code"): the mask the coarse levels were built from, an earlier one."""
    mks = [O.Mask(mask)]
    solid = O.Mask(stale_mask if (wrong == "stale_code" and stale_mask is not None) else mask).solid
    for n in ns[1:]:
        solid = coarsen(solid, wrong)
        full = np.zeros((n + 2,) * 3, np.float64)
        full[I, I, I] = solid
        mks.append(O.Mask(full, "ghost_fluid" if wrong == "coarse_ghost_fluid" else None, slabs))
    return mks


def smooth(z, r, mk, wrong=None, level=0, first=False):
    """One masked sweep: z' = z + c_s (r - A_m z) on fluid cells, +0 on solid ones, then set_bnd(0, z'). first: the sweep
    from z = +0, which the SPEC's expression makes T(0) + c_s r."""
    if wrong == "coarse_unmasked" and level > 0:
        return G.smooth(z, r)
    T = z.dtype.type
    cs = T(1.0 / 7.0)
    zn = np.zeros_like(z)
    val = cs * r if (first and wrong == "first_smooth_no_zero") else z[I, I, I] + cs * (r - O.apply_A(z, mk))
    zn[I, I, I] = val if wrong == "solids_not_zeroed" else np.where(mk.solid, T(0), val)
    return R.set_bnd(0, zn)


def vcycle(r, mask, nu, max_levels=0, nu_c=8, wrong=None, slabs=1, stale_mask=None):
    """z = V_m(0, r) of SPEC §16. r: interior-shaped (N, N, N); mask: (N+2)^3. Returns the whole field z."""
    ns = G.levels(r.shape[0], max_levels)
    mks = level_masks(mask, ns, wrong, slabs, stale_mask)

    def cycle(r, l):
        T = r.dtype.type
        mk = mks[l]
        last = l == len(ns) - 1
        z = np.zeros(tuple(n + 2 for n in r.shape), r.dtype)
        for n in range(nu_c if last else nu):
            z = smooth(z, r, mk, wrong, l, first=n == 0)
        if last:
            return z
        e = r - O.apply_A(z, mk)
        if wrong != "e_not_zeroed":
            e = np.where(mk.solid, T(0), e)
        zc = cycle(G.restrict(e), l + 1)
        par = (np.arange(1, r.shape[0] + 1) + 1) // 2
        val = z[I, I, I] + zc[np.ix_(par, par, par)]
        z[I, I, I] = val if wrong == "prolong_into_solids" else np.where(mk.solid, T(0), val)
        R.set_bnd(0, z)
        for _ in range(nu):
            z = smooth(z, r, mk, wrong, l)
        return z

    with np.errstate(all="ignore"):
        return cycle(r, 0)


def project_cg(u, v, w, mask, tol, max_iters, nu, max_levels=0, nu_c=8, slabs=1, history=None, wrong=None,
               stale_mask=None, M=None, ops=S3.SPEC):
    """SPEC §16 "Solve": §15's masked project_cg with z = V_m(0, r) where it says z = M(r), on copies of u, v, w. Returns
    the dict of pressure_cg_ref.project_cg. M: another z = M(r) in the V-cycle's place (jacobi:8 for the counts)."""
    M = M or (lambda r: vcycle(r, mask, nu, max_levels, nu_c, wrong, slabs, stale_mask))
    dtype = u.dtype
    T = dtype.type
    mk = O.Mask(mask)
    u, v, w = u.copy(), v.copy(), w.copy()
    with np.errstate(all="ignore"):
        p, div = O.divergence(u, v, w, mk, None, ops)
        s = R.tree_sum(div[I, I, I].astype(np.float64), dtype, slabs)
        mu = T(s / float(mk.n_fluid)) if mk.n_fluid else T(0)
        r = np.where(mk.solid, T(0), div[I, I, I] - mu)
        rho0 = last = R.dot(r, r, dtype, slabs)
        status, iters = MAX_ITERS, 0
        if rho0 == 0.0:
            status = CONVERGED
        elif not math.isfinite(rho0):
            status = BREAKDOWN
        else:
            z = M(r)
            gamma = R.dot(r, z[I, I, I], dtype, slabs)
            if not gamma > 0.0:
                status = BREAKDOWN
            else:
                d = np.zeros_like(u)
                d[I, I, I] = z[I, I, I]
                R.set_bnd(0, d)
                for n in range(max_iters):
                    q = O.apply_A(d, mk)
                    delta = R.dot(d[I, I, I], q, dtype, slabs)
                    if not delta > 0.0:
                        status = BREAKDOWN
                        break
                    aT = T(gamma / delta)
                    p[I, I, I] = p[I, I, I] + aT * d[I, I, I]
                    r = r - aT * q
                    rho_new = last = R.dot(r, r, dtype, slabs)
                    iters = n + 1
                    if history is not None:
                        history.append(rho_new)
                    if not math.isfinite(rho_new):
                        status = BREAKDOWN
                        break
                    if rho_new <= (tol * tol) * rho0:
                        status = CONVERGED
                        break
                    z = M(r)
                    gamma_new = R.dot(r, z[I, I, I], dtype, slabs)
                    if not gamma_new > 0.0:
                        status = BREAKDOWN
                        break
                    bT = T(gamma_new / gamma)
                    d[I, I, I] = z[I, I, I] + bT * d[I, I, I]
                    R.set_bnd(0, d)
                    gamma = gamma_new
        R.set_bnd(0, p)
        O.subtract_gradient(u, v, w, p, mk)
        rel = 0.0 if rho0 == 0.0 else math.sqrt(last / rho0) if last / rho0 >= 0 else float("nan")
    return {"u": u, "v": v, "w": w, "p": p, "div": div, "status": status, "iterations": iters, "rel_residual": rel}


def vel_step(f, mask, K, dt, visc, tol, max_iters, mg):
    """SPEC §3 vel_step on copies of the velocity fields of f, both projections the solve above with the setting mg
    (§15 "Steps"; no bound sources). Returns the second projection's outcome."""
    u, v, w, u0, v0, w0 = (f[n].copy() for n in ("u", "v", "w", "u0", "v0", "w0"))
    T = u.dtype.type
    Nf = T(u.shape[0] - 2)
    for x, s in ((u, u0), (v, v0), (w, w0)):
        S3.add_source(x, s, dt)
    u, u0, v, v0, w, w0 = u0, u, v0, v, w0, w
    a = ((T(dt) * T(visc)) * Nf) * Nf
    for b, x, x0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        S3.lin_solve(b, x, x0, a, T(1) + T(6) * a, K)
    out = project_cg(u, v, w, mask, tol, max_iters, *mg)
    u0, v0, w0 = out["u"], out["v"], out["w"]
    u, v, w = (np.zeros_like(u0) for _ in range(3))
    for b, d, d0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        S3.advect(b, d, d0, u0, v0, w0, dt)
    return project_cg(u, v, w, mask, tol, max_iters, *mg)
