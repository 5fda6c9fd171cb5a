"""numpy reference of docs/SPEC.md §15 "Solid obstacles", written from the SPEC text on the pieces of
tests/pressure_cg_ref.py and tests/pressure_pcg_ref.py (set_bnd, the §10 sums, z = M(r)). It does not call the library.
Fields and the mask are (N+2, N+2, N+2) arrays indexed [k, j, i]; every per-cell expression is one numpy operation per
SPEC operation on the dtype, every face rule a select (np.where) on values that are all evaluated.

`wrong` names one deliberately wrong reading of §15 (WRONG): tests/test_obstacles_ref.py shows for each of them a case
whose result it changes, so that a test against this reference tells that reading from the SPEC's.
"""
import math

import numpy as np

import pressure_cg_ref as R
import pressure_pcg_ref as Q
import stable_ref as S3

I, P, M = R.I, R.P, R.M
CONVERGED, MAX_ITERS, BREAKDOWN = R.CONVERGED, R.MAX_ITERS, R.BREAKDOWN
# the six faces of a cell as (name, index of the neighbour [k, j, i]): low and high of i, j, k
FACES = (("ilo", (I, I, M)), ("ihi", (I, I, P)), ("jlo", (I, M, I)), ("jhi", (I, P, I)), ("klo", (M, I, I)),
         ("khi", (P, I, I)))
WRONG = ("closed_zero", "div_stored", "mu_n3", "grad_unmasked", "solids_not_zeroed", "faces_swapped", "nan_solid",
         "ghost_fluid", "r_not_zeroed")
# wrong readings that only special values (zeros of either sign, subnormals, non-finite values) in the fluid tell from the
# SPEC's: tests/test_obstacle_special_inputs_ref.py. FaceMinus is an `ops` (stable_ref.Ops with neg as T(0) - x).
SPECIAL_WRONG = ("grad_add", "solid_as_product")


def solid_cells(mask, wrong=None):
    """solid(c) on all (N+2)^3 entries: an interior cell with mask > 0 in the dtype (NaN, -0, negatives: fluid); shell
    cells are never solid."""
    s = np.zeros(mask.shape, bool)
    with np.errstate(invalid="ignore"):
        s[I, I, I] = ~(mask[I, I, I] <= 0) if wrong == "nan_solid" else mask[I, I, I] > 0
    return s


class Mask:
    """What §15 derives from a mask: fluid (interior-shaped), n_fluid and the closed faces of every interior cell."""

    def __init__(self, mask, wrong=None, slabs=1):
        solid = solid_cells(mask, wrong)
        self.solid = solid[I, I, I]
        self.fluid = ~self.solid
        self.n_fluid = int(self.fluid.sum())
        self.closed = {name: solid[nb].copy() for name, nb in FACES}
        if wrong == "ghost_fluid":  # the neighbours across a slab boundary taken as fluid
            nzl = self.solid.shape[0] // slabs
            for s in range(1, slabs):
                self.closed["klo"][s * nzl] = False
                self.closed["khi"][s * nzl - 1] = False
        if wrong == "faces_swapped":
            c = self.closed
            self.closed = {"ilo": c["ihi"], "ihi": c["ilo"], "jlo": c["jhi"], "jhi": c["jlo"], "klo": c["khi"],
                           "khi": c["klo"]}

    def eff(self, x, face, sign=1, ops=S3.SPEC):
        """eff (sign 1) / effn (sign -1) of one face on all interior cells: the cell itself where the face is closed,
        the neighbour as stored where it is open."""
        nb = dict(FACES)[face]
        own = x[I, I, I] if sign == 1 else ops.neg(x[I, I, I])
        return np.where(self.closed[face], own, x[nb])

    def zeroed(self, val, wrong=None):
        """solid ? +0 : val."""
        if wrong == "solid_as_product":
            with np.errstate(invalid="ignore"):
                return val * self.fluid.astype(val.dtype)
        return np.where(self.solid, val.dtype.type(0), val)


def divergence(u, v, w, mk, wrong=None, ops=S3.SPEC):
    """§15 step 1: (p, div) with both set_bnd(0, .)."""
    T = u.dtype.type
    N = u.shape[0] - 2
    c_div = T(-0.5) * (T(1) / T(N))
    e = (lambda x, f: x[dict(FACES)[f]]) if wrong == "div_stored" else (lambda x, f: mk.eff(x, f, -1, ops))
    div = np.zeros_like(u)
    val = c_div * (((e(u, "ihi") - e(u, "ilo")) + (e(v, "jhi") - e(v, "jlo"))) + (e(w, "khi") - e(w, "klo")))
    div[I, I, I] = mk.zeroed(val, wrong)
    R.set_bnd(0, div)
    return np.zeros_like(u), div


def apply_A(x, mk, wrong=None):
    """§15 step 3 on the interior cells."""
    T = x.dtype.type
    e = (lambda f: np.where(mk.closed[f], T(0), x[dict(FACES)[f]])) if wrong == "closed_zero" else (lambda f: mk.eff(x, f))
    val = T(6) * x[I, I, I] - (((e("ilo") + e("ihi")) + (e("jlo") + e("jhi"))) + (e("klo") + e("khi")))
    return np.where(mk.solid, T(0), val)


def subtract_gradient(u, v, w, p, mk, wrong=None):
    """§15 step 5, in place."""
    T = u.dtype.type
    N = u.shape[0] - 2
    c_grad = T(0.5) * T(N)
    e = (lambda f: p[dict(FACES)[f]]) if wrong == "grad_unmasked" else (lambda f: mk.eff(p, f))
    for x, lo, hi in ((u, "ilo", "ihi"), (v, "jlo", "jhi"), (w, "klo", "khi")):
        if wrong == "grad_add":
            val = x[I, I, I] + c_grad * (e(lo) - e(hi))
        else:
            val = x[I, I, I] - c_grad * (e(hi) - e(lo))
        x[I, I, I] = val if wrong == "solids_not_zeroed" else mk.zeroed(val, wrong)
    R.set_bnd(1, u)
    R.set_bnd(2, v)
    R.set_bnd(3, w)


def project_cg(u, v, w, mask, tol, max_iters, m=0, slabs=1, history=None, wrong=None, ops=S3.SPEC):
    """SPEC §15 masked project_cg (m Jacobi sweeps of §11.2 as the preconditioner; 0: §11) on copies of u, v, w. Returns
    the dict of pressure_cg_ref.project_cg."""
    dtype = u.dtype
    T = dtype.type
    N = u.shape[0] - 2
    mk = Mask(mask, wrong, slabs)
    u, v, w = u.copy(), v.copy(), w.copy()
    pc = m > 0
    with np.errstate(all="ignore"):
        p, div = divergence(u, v, w, mk, wrong, ops)
        s = R.tree_sum(div[I, I, I].astype(np.float64), dtype, slabs)
        count = N ** 3 if wrong == "mu_n3" else mk.n_fluid
        mu = T(s / float(count)) if count else T(0)
        r = div[I, I, I] - mu
        if wrong != "r_not_zeroed":
            r = np.where(mk.solid, T(0), r)
        rho0 = last = R.dot(r, r, dtype, slabs)
        status, iters = MAX_ITERS, 0
        d = np.zeros_like(u)
        go = False
        if rho0 == 0.0:
            status = CONVERGED
        elif not math.isfinite(rho0):
            status = BREAKDOWN
        elif pc:
            z = Q.precondition(r, m)
            gamma = R.dot(r, z[I, I, I], dtype, slabs)
            if not gamma > 0.0:
                status = BREAKDOWN
            else:
                d[I, I, I] = z[I, I, I]
                go = True
        else:
            d[I, I, I] = r
            gamma = rho0
            go = True
        if go:
            R.set_bnd(0, d)
            for n in range(max_iters):
                q = apply_A(d, mk, wrong)
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
                if pc:
                    z = Q.precondition(r, m)
                    gamma_new = R.dot(r, z[I, I, I], dtype, slabs)
                    if not gamma_new > 0.0:
                        status = BREAKDOWN
                        break
                    lead = z[I, I, I]
                else:
                    gamma_new, lead = rho_new, r
                bT = T(gamma_new / gamma)
                d[I, I, I] = lead + bT * d[I, I, I]
                R.set_bnd(0, d)
                gamma = gamma_new
        R.set_bnd(0, p)
        subtract_gradient(u, v, w, p, mk, wrong)
        rel = 0.0 if rho0 == 0.0 else math.sqrt(last / rho0) if last / rho0 >= 0 else float("nan")
    return {"u": u, "v": v, "w": w, "p": p, "div": div, "status": status, "iterations": iters, "rel_residual": rel}


def poisson_residual(p, div, mask, slabs=1, wrong=None):
    """sqrt(sum e.e / sum div.div) under a mask: e = div - A p on fluid cells, +0 on solid ones; div.div as stored."""
    T = p.dtype.type
    mk = Mask(mask, wrong, slabs)
    with np.errstate(all="ignore"):
        e = np.where(mk.solid, T(0), div[I, I, I] - apply_A(p, mk, wrong))
        ee = R.dot(e, e, p.dtype, slabs)
        dd = R.dot(div[I, I, I], div[I, I, I], p.dtype, slabs)
        if dd == 0.0:
            return 0.0
        x = ee / dd
        return math.sqrt(x) if x >= 0 else float("nan")


def zero_solids(x, mask):
    """The end of a masked dens_step, in place: x = +0 on solid cells, then set_bnd(0, x)."""
    x[I, I, I] = np.where(Mask(mask).solid, x.dtype.type(0), x[I, I, I])
    R.set_bnd(0, x)
    return x


def vel_step(f, mask, K, dt, visc, tol, max_iters, m=0, sources=None):
    """SPEC §3 vel_step on copies of the velocity fields of f with both projections the masked one (§15 "Steps");
    diffusion and advection unaware of the mask. sources: bound sources, which replace the x0 fields first. Returns the
    second projection's outcome."""
    u, v, w, u0, v0, w0 = (f[n].copy() for n in ("u", "v", "w", "u0", "v0", "w0"))
    if sources:
        u0, v0, w0 = (sources[n].copy() for n in ("u0", "v0", "w0"))
    T = u.dtype.type
    Nf = T(u.shape[0] - 2)
    for x, s in ((u, u0), (v, v0), (w, w0)):
        S3.add_source(x, s, dt)
    u, u0, v, v0, w, w0 = u0, u, v0, v, w0, w
    a = ((T(dt) * T(visc)) * Nf) * Nf
    for b, x, x0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        S3.lin_solve(b, x, x0, a, T(1) + T(6) * a, K)
    out = project_cg(u, v, w, mask, tol, max_iters, m)
    u0, v0, w0 = out["u"], out["v"], out["w"]
    u, v, w = (np.zeros_like(u0) for _ in range(3))
    for b, d, d0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        S3.advect(b, d, d0, u0, v0, w0, dt)
    return project_cg(u, v, w, mask, tol, max_iters, m)


def dens_step(dens, dens0, u, v, w, mask, K, dt, diff, source=None):
    """SPEC §3 dens_step on copies, ended by zero_solids. Returns the density."""
    x, x0 = dens.copy(), (source if source is not None else dens0).copy()
    T = x.dtype.type
    Nf = T(x.shape[0] - 2)
    S3.add_source(x, x0, dt)
    x, x0 = x0, x
    a = ((T(dt) * T(diff)) * Nf) * Nf
    S3.lin_solve(0, x, x0, a, T(1) + T(6) * a, K)
    x, x0 = x0, x
    S3.advect(0, x, x0, u, v, w, dt)
    return zero_solids(x, mask)
