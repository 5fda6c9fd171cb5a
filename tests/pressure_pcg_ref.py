"""numpy reference of docs/SPEC.md §11.2 "Preconditioned CG", written from the SPEC text. It does not call the library.
Built from the pieces of tests/pressure_cg_ref.py (apply_A, dot, tree_sum, divergence, subtract_gradient, set_bnd) and
§3's lin_solve as tests/stable_ref.py states it; fields, sums and scalars follow the conventions of pressure_cg_ref.
"""
import math

import numpy as np

import pressure_cg_ref as R
import stable_ref as S3

I = R.I
CONVERGED, MAX_ITERS, BREAKDOWN = R.CONVERGED, R.MAX_ITERS, R.BREAKDOWN


def precondition(r, m):
    """z = M(r): z = +0 on all S^3 entries, then lin_solve(0, z, r, 1, 6, m) exactly as §3. r: interior-shaped; only
    interior cells of the right-hand side are read. Returns the whole field z, shells included."""
    N = r.shape[0]
    rhs = np.zeros((N + 2,) * 3, r.dtype)
    rhs[I, I, I] = r
    z = np.zeros_like(rhs)
    S3.lin_solve(0, z, rhs, 1, 6, m)
    return z


def project_cg(u, v, w, tol, max_iters, m, slabs=1, history=None):
    """SPEC §11.2 project_cg with m Jacobi sweeps as the preconditioner, on copies of u, v, w; m = 0 is §11 itself
    (pressure_cg_ref.project_cg). Returns the same dict. history (a list) receives rho' after every iteration."""
    if m == 0:
        return R.project_cg(u, v, w, tol, max_iters, slabs=slabs, history=history)
    assert m >= 1
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
            z = precondition(r, m)
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
                    z = precondition(r, m)
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
