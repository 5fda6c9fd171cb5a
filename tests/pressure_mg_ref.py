"""numpy reference of docs/SPEC.md §11.3 "Multigrid V-cycle preconditioner", written from the SPEC text. It does not call
the library. Built from the pieces of tests/pressure_cg_ref.py (apply_A, dot, tree_sum, divergence, subtract_gradient,
set_bnd); fields, sums and scalars follow its conventions: one numpy operation per SPEC operation on the dtype.

`variant` names a deliberately wrong V-cycle (tests/test_pressure_mg_ref.py shows which GPU case tells each from the
right one); None is the SPEC.
"""
import math

import numpy as np

import pressure_cg_ref as R

I = R.I
CONVERGED, MAX_ITERS, BREAKDOWN = R.CONVERGED, R.MAX_ITERS, R.BREAKDOWN
VARIANTS = ("restrict_assoc", "quarter", "parent_floor", "no_bnd_after_prolong", "coarse_as_nu", "coarsen_to_2",
            "extra_post_sweep", "stale_after_prolong")


def levels(N, max_levels=0, min_coarse=4):
    """[n_0, n_1, ...]: n_{l+1} = n_l / 2 while n_l is even, n_l / 2 >= 4 and (max_levels == 0 or l + 1 < max_levels)."""
    n = [N]
    while n[-1] % 2 == 0 and n[-1] // 2 >= min_coarse and (max_levels == 0 or len(n) < max_levels):
        n.append(n[-1] // 2)
    return n


def admissible_levels(N, P):
    """The largest max_levels a context of P slabs admits: every n_l with l >= 1 divisible by P."""
    n = levels(N, 0)
    ok = 1
    while ok < len(n) and n[ok] % P == 0:
        ok += 1
    return ok


def smooth(z, r):
    """One sweep z -> z' = z + c_s (r - A z) on interior cells, then set_bnd(0, z'). r: interior-shaped."""
    T = z.dtype.type
    cs = T(1.0 / 7.0)
    zn = np.zeros_like(z)
    zn[I, I, I] = z[I, I, I] + cs * (r - R.apply_A(z))
    return R.set_bnd(0, zn)


def first_sweep(r):
    """The first sweep from z = +0 as the SPEC allows it to be evaluated: T(0) + c_s r, then set_bnd."""
    T = r.dtype.type
    z = np.zeros(tuple(n + 2 for n in r.shape), r.dtype)
    z[I, I, I] = T(0) + T(1.0 / 7.0) * r
    return R.set_bnd(0, z)


def restrict(e, variant=None):
    """rc = half * (((e000 + e100) + (e010 + e110)) + ((e001 + e101) + (e011 + e111))) over the eight children;
    e, rc interior-shaped [k, j, i]."""
    T = e.dtype.type
    lo, hi = slice(0, None, 2), slice(1, None, 2)  # 0-based children 2I-2, 2I-1 of 1-based coarse I
    c = lambda k, j, i: e[k, j, i]
    if variant == "restrict_assoc":  # a flat left-to-right sum
        s = c(lo, lo, lo)
        for k, j, i in ((lo, lo, hi), (lo, hi, lo), (lo, hi, hi), (hi, lo, lo), (hi, lo, hi), (hi, hi, lo), (hi, hi, hi)):
            s = s + c(k, j, i)
    else:
        s = ((c(lo, lo, lo) + c(lo, lo, hi)) + (c(lo, hi, lo) + c(lo, hi, hi))) + \
            ((c(hi, lo, lo) + c(hi, lo, hi)) + (c(hi, hi, lo) + c(hi, hi, hi)))
    return (T(0.25) if variant == "quarter" else T(0.5)) * s


def prolong_add(z, zc, variant=None):
    """z[i, j, k] += zc[(i+1)/2, (j+1)/2, (k+1)/2] on the interior, then set_bnd(0, z). In place."""
    n = z.shape[0] - 2
    idx = np.arange(1, n + 1)
    par = idx // 2 if variant == "parent_floor" else (idx + 1) // 2
    z[I, I, I] = z[I, I, I] + zc[np.ix_(par, par, par)]
    if variant != "no_bnd_after_prolong":
        R.set_bnd(0, z)
    return z


def vcycle(r, nu, max_levels=0, nu_c=8, variant=None, z_init=None, slabs=1, _l=0, _ns=None):
    """z = V(0, r) of SPEC §11.3. r: interior-shaped (N, N, N). Returns the whole field z, shells included.
    z_init: the iterate the fine level starts from in place of +0 (a mutant: a z that was not zeroed). slabs with
    variant "stale_after_prolong": every slab runs the first post-sweep of a level with the ghost planes of z as they
    were before step 5 (the exchange after the correction left out)."""
    if _ns is None:
        _ns = levels(r.shape[0], max_levels, 2 if variant == "coarsen_to_2" else 4)
    last = _l == len(_ns) - 1
    s = nu if (not last or variant == "coarse_as_nu") else nu_c
    z = np.zeros(tuple(n + 2 for n in r.shape), r.dtype) if z_init is None else z_init.copy()
    for _ in range(s):
        z = smooth(z, r)
    if last:
        return z
    e = r - R.apply_A(z)
    zc = vcycle(restrict(e, variant), nu, max_levels, nu_c, variant, None, slabs, _l + 1, _ns)
    before = z.copy()
    prolong_add(z, zc, variant)
    for t in range(nu + (1 if variant == "extra_post_sweep" else 0)):
        if variant == "stale_after_prolong" and t == 0 and slabs > 1:
            n = r.shape[0]
            assert n % slabs == 0
            nzl, nxt = n // slabs, np.zeros_like(z)
            for g in range(slabs):
                a, b = 1 + g * nzl, 1 + (g + 1) * nzl  # the slab's planes [a, b); wall slabs own the shell planes
                lo, hi = (0 if g == 0 else a), (n + 2 if g == slabs - 1 else b)
                seen = before.copy()
                seen[lo:hi] = z[lo:hi]
                nxt[lo:hi] = smooth(seen, r)[lo:hi]
            z = nxt
        else:
            z = smooth(z, r)
    return z


def project_cg(u, v, w, tol, max_iters, nu, max_levels=0, nu_c=8, slabs=1, history=None, M=None):
    """SPEC §11.2 steps 1-6 with M = V(0, .) on copies of u, v, w; the dict of pressure_cg_ref.project_cg. history (a
    list) receives rho' after every iteration. M: another z = M(r) in the V-cycle's place (a mutant)."""
    M = M or (lambda r: vcycle(r, nu, max_levels, nu_c))
    dtype = u.dtype
    T = dtype.type
    N = u.shape[0] - 2
    u, v, w = u.copy(), v.copy(), w.copy()
    with np.errstate(all="ignore"):
        p, div = R.divergence(u, v, w)
        s = R.tree_sum(div[I, I, I].astype(np.float64), dtype, slabs)
        mu = T(s / float(N) ** 3)
        r = div[I, I, I] - mu
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
                    q = R.apply_A(d)
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
        R.subtract_gradient(u, v, w, p)
        rel = 0.0 if rho0 == 0.0 else math.sqrt(last / rho0) if last / rho0 >= 0 else float("nan")
    return {"u": u, "v": v, "w": w, "p": p, "div": div, "status": status, "iterations": iters, "rel_residual": rel}
