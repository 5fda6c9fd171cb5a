"""numpy reference of docs/SPEC.md §11 "Conjugate-gradient projection", written from the SPEC text. It does not call the
library. Fields are (N+2, N+2, N+2) arrays indexed [k, j, i] of float32 or float64. Every per-cell expression is one
numpy operation per SPEC operation on that dtype (numpy rounds each one, no contraction); every inner product is the
§10 sum tree of tests/diagnostics_ref.py over terms multiplied in double; alpha, beta and the stop tests are Python
floats (doubles), rounded to the dtype once where a cell uses them.
"""
import math

import numpy as np

import diagnostics_ref as D

I, P, M = slice(1, -1), slice(2, None), slice(None, -2)
CONVERGED, MAX_ITERS, BREAKDOWN = 0, 1, 2


def set_bnd(b, x):
    """SPEC §3 set_bnd, in place: faces, then the 12 edges, then the 8 corners."""
    T = x.dtype.type
    sx, sy, sz = (T(-1) if b == a else T(1) for a in (1, 2, 3))
    half, third = T(0.5), T(1.0 / 3.0)
    x[I, I, 0] = sx * x[I, I, 1]
    x[I, I, -1] = sx * x[I, I, -2]
    x[I, 0, I] = sy * x[I, 1, I]
    x[I, -1, I] = sy * x[I, -2, I]
    x[0, I, I] = sz * x[1, I, I]
    x[-1, I, I] = sz * x[-2, I, I]
    for a, an in ((0, 1), (-1, -2)):
        for c, cn in ((0, 1), (-1, -2)):
            x[c, a, I] = half * (x[c, an, I] + x[cn, a, I])  # x[i, J, K]: lower axis (j) first
            x[c, I, a] = half * (x[c, I, an] + x[cn, I, a])  # x[I, j, K]
            x[I, c, a] = half * (x[I, c, an] + x[I, cn, a])  # x[I, J, k]
    for k, kn in ((0, 1), (-1, -2)):
        for j, jn in ((0, 1), (-1, -2)):
            for i, i_n in ((0, 1), (-1, -2)):
                x[k, j, i] = third * ((x[k, j, i_n] + x[k, jn, i]) + x[kn, j, i])
    return x


def apply_A(x):
    """(A x) on the interior cells, neighbours as stored."""
    T = x.dtype.type
    return T(6) * x[I, I, I] - (((x[I, I, M] + x[I, I, P]) + (x[I, M, I] + x[I, P, I])) + (x[M, I, I] + x[P, I, I]))


def tree_sum(terms, dtype, slabs=1):
    """§10 sum of (N, N, N) double terms [k, j, i]; through `slabs` emulated slabs the plane records of each are
    computed apart and folded in global k order."""
    N = terms.shape[0]
    assert N % slabs == 0
    nzl = N // slabs
    W = D.vec_width(dtype)
    with np.errstate(all="ignore"):
        recs = [D.plane_partials(terms[s * nzl:(s + 1) * nzl], W) for s in range(slabs)]
        return D.total(np.concatenate(recs))


def dot(a, b, dtype, slabs=1):
    """sum a.b over interior-shaped arrays: converted to double first, multiplied in double, summed by the tree."""
    with np.errstate(all="ignore"):
        return tree_sum(a.astype(np.float64) * b.astype(np.float64), dtype, slabs)


def divergence(u, v, w):
    """First half of §3 project: (p, div) with both set_bnd(0, .)."""
    T = u.dtype.type
    N = u.shape[0] - 2
    c_div = T(-0.5) * (T(1) / T(N))
    div = np.zeros_like(u)
    div[I, I, I] = c_div * (((u[I, I, P] - u[I, I, M]) + (v[I, P, I] - v[I, M, I])) + (w[P, I, I] - w[M, I, I]))
    set_bnd(0, div)
    return np.zeros_like(u), div


def subtract_gradient(u, v, w, p):
    """Second half of §3 project, in place."""
    T = u.dtype.type
    N = u.shape[0] - 2
    c_grad = T(0.5) * T(N)
    u[I, I, I] = u[I, I, I] - c_grad * (p[I, I, P] - p[I, I, M])
    v[I, I, I] = v[I, I, I] - c_grad * (p[I, P, I] - p[I, M, I])
    w[I, I, I] = w[I, I, I] - c_grad * (p[P, I, I] - p[M, I, I])
    set_bnd(1, u)
    set_bnd(2, v)
    set_bnd(3, w)


def project_cg(u, v, w, tol, max_iters, slabs=1, history=None):
    """SPEC §11 project_cg on copies of u, v, w. Returns a dict: u, v, w, p, div, status, iterations, rel_residual.
    history (a list) receives rho after every iteration."""
    dtype = u.dtype
    T = dtype.type
    N = u.shape[0] - 2
    u, v, w = u.copy(), v.copy(), w.copy()
    with np.errstate(all="ignore"):
        p, div = divergence(u, v, w)
        s = tree_sum(div[I, I, I].astype(np.float64), dtype, slabs)
        mu = T(s / float(N) ** 3)
        r = div[I, I, I] - mu
        d = np.zeros_like(u)
        d[I, I, I] = r
        set_bnd(0, d)
        rho0 = rho = last = dot(r, r, dtype, slabs)
        status, iters = MAX_ITERS, 0
        if rho0 == 0.0:
            status = CONVERGED
        elif not math.isfinite(rho0):
            status = BREAKDOWN
        else:
            for n in range(max_iters):
                q = apply_A(d)
                delta = dot(d[I, I, I], q, dtype, slabs)
                if not delta > 0.0:
                    status = BREAKDOWN
                    break
                aT = T(rho / delta)
                p[I, I, I] = p[I, I, I] + aT * d[I, I, I]
                r = r - aT * q
                rho_new = last = dot(r, r, dtype, slabs)
                iters = n + 1
                if history is not None:
                    history.append(rho_new)
                if not math.isfinite(rho_new):
                    status = BREAKDOWN
                    break
                if rho_new <= (tol * tol) * rho0:
                    status = CONVERGED
                    break
                bT = T(rho_new / rho)
                d[I, I, I] = r + bT * d[I, I, I]
                set_bnd(0, d)
                rho = rho_new
        set_bnd(0, p)
        subtract_gradient(u, v, w, p)
        rel = 0.0 if rho0 == 0.0 else math.sqrt(last / rho0) if last / rho0 >= 0 else float("nan")
    return {"u": u, "v": v, "w": w, "p": p, "div": div, "status": status, "iterations": iters, "rel_residual": rel}


def poisson_residual(p, div, slabs=1):
    """sqrt(sum e.e / sum div.div), e = div - A p in the dtype; 0 when sum div.div == 0."""
    with np.errstate(all="ignore"):
        e = div[I, I, I] - apply_A(p)
        ee = dot(e, e, p.dtype, slabs)
        dd = dot(div[I, I, I], div[I, I, I], p.dtype, slabs)
        if dd == 0.0:
            return 0.0
        x = ee / dd
        return math.sqrt(x) if x >= 0 else float("nan")


def project_jacobi(u, v, w, K):
    """§3 project with K Jacobi sweeps, on copies: the same dict as project_cg (without the solve's status)."""
    T = u.dtype.type
    u, v, w = u.copy(), v.copy(), w.copy()
    p, div = divergence(u, v, w)
    inv = T(1) / T(6)
    for _ in range(K):
        pn = np.zeros_like(p)
        pn[I, I, I] = (div[I, I, I] + T(1) * (((p[I, I, M] + p[I, I, P]) + (p[I, M, I] + p[I, P, I]))
                                              + (p[M, I, I] + p[P, I, I]))) * inv
        p = set_bnd(0, pn)
    subtract_gradient(u, v, w, p)
    return {"u": u, "v": v, "w": w, "p": p, "div": div}


def smooth_velocity(N, dtype):
    """The smooth test field of SPEC §11.1: evaluated in double on all (N+2)^3 entries, rounded, then set_bnd."""
    x = (np.arange(N + 2) - 0.5) / N
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    A = 0.5 / (0.1 * N)
    pi = np.pi
    u = A * np.sin(2 * pi * X) * np.cos(2 * pi * Y) + 0.3 * A * np.sin(3 * pi * X) * np.cos(pi * Z)
    v = -A * np.cos(2 * pi * X) * np.sin(2 * pi * Y) + 0.2 * A * np.sin(pi * Y)
    w = 0.25 * A * np.sin(2 * pi * Z) * np.cos(pi * X)
    u, v, w = (np.ascontiguousarray(f.astype(dtype)) for f in (u, v, w))
    set_bnd(1, u)
    set_bnd(2, v)
    set_bnd(3, w)
    return u, v, w
