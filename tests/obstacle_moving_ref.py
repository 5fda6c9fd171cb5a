"""numpy reference of docs/SPEC.md §19 "Moving solids", written from the SPEC text on the pieces of
tests/obstacles_ref.py (Mask, eff, the masked A, set_bnd), tests/obstacles_mg_ref.py (the masked V-cycle),
tests/pressure_pcg_ref.py (z = M(r)) and tests/obstacle_transport_ref.py (the b = 0 forms, dens_step). It does not call
the library. Fields, the mask and the three solid-velocity fields are (N+2)^3 arrays [k, j, i]; every per-cell
expression is one numpy operation per SPEC operation on the dtype, every face, sample and solid rule a select
(np.where) on values that are all evaluated.

`wrong` names one deliberately wrong reading of §19 (WRONG): tests/test_obstacle_moving_ref.py shows for each of them a
case whose result it changes. `slabs`: the k-slabs of a decomposition, for the §10 sums and for the wrong reading
"xs_ghost_stale", in which a slab sees +0 where the solid velocity lies across a slab boundary.
"""
import math

import numpy as np

import forces_ref as F
import obstacle_transport_ref as TR
import obstacles_mg_ref as OM
import obstacles_ref as OB
import pressure_cg_ref as R
import pressure_pcg_ref as Q
import stable_ref as S3

I = R.I
I3 = (I, I, I)
FACES = dict(OB.FACES)
AXIS = TR.AXIS
OPPOSITE = {"ilo": "ihi", "ihi": "ilo", "jlo": "jhi", "jhi": "jlo", "klo": "khi", "khi": "klo"}
CONVERGED, MAX_ITERS, BREAKDOWN = R.CONVERGED, R.MAX_ITERS, R.BREAKDOWN
WRONG = ("no_doubling", "plus_x", "xs_at_c", "wrong_axis", "no_slip", "nb_swapped", "solids_zero_after_project",
         "solids_set_by_sweep", "solids_set_by_advect", "wv_at_c", "velocity_of_i0", "fluid_entry", "xs_ghost_stale",
         "effv_b0")


class Moving(OB.Mask):
    """obstacles_ref.Mask with the solid velocity vs = (us, vs, ws): effv of one face on all interior cells."""

    def __init__(self, mask, vs, wrong=None, slabs=1):
        super().__init__(mask)
        self.vs, self.wrong, self.slabs = vs, wrong, slabs

    def solid_velocity(self, axis, face):
        """xs_axis[nb] for the neighbour across `face`, interior-shaped."""
        wrong = self.wrong
        if wrong == "wrong_axis":
            axis = axis % 3 + 1
        xs = self.vs[axis - 1]
        if wrong == "xs_at_c":
            return xs[I3]
        s = xs[FACES[OPPOSITE[face] if wrong == "nb_swapped" else face]]
        if wrong == "xs_ghost_stale" and face in ("klo", "khi"):  # the plane across a slab boundary reads +0
            s = s.copy()
            nzl = s.shape[0] // self.slabs
            for b in range(1, self.slabs):
                s[b * nzl if face == "klo" else b * nzl - 1] = 0
        return s

    def effv(self, x, face, axis=None):
        """(xs[nb] + xs[nb]) - x[c] across a closed face, x[nb] otherwise; xs of the face's axis (axis: of another)."""
        wrong = self.wrong
        s = self.solid_velocity(axis or AXIS[face], face)
        own = x[I3]
        with np.errstate(invalid="ignore", over="ignore"):
            if wrong == "no_doubling":
                ghost = s - own
            elif wrong == "plus_x":
                ghost = (s + s) + own
            else:
                ghost = (s + s) - own
            if wrong == "fluid_entry":  # the select as a blend: the ghost of an open face is an operand too
                return x[FACES[face]] + self.closed[face].astype(own.dtype) * (ghost - x[FACES[face]])
        return np.where(self.closed[face], ghost, x[FACES[face]])


def divergence(u, v, w, mk):
    """§19 masked divergence: (p, div) with both set_bnd(0, .)."""
    T = u.dtype.type
    N = u.shape[0] - 2
    c_div = T(-0.5) * (T(1) / T(N))
    e = mk.effv
    div = np.zeros_like(u)
    val = c_div * (((e(u, "ihi") - e(u, "ilo")) + (e(v, "jhi") - e(v, "jlo"))) + (e(w, "khi") - e(w, "klo")))
    div[I3] = mk.zeroed(val)
    R.set_bnd(0, div)
    return np.zeros_like(u), div


def subtract_gradient(u, v, w, p, mk):
    """§19 gradient subtraction, in place: §15's on fluid cells, the solid's velocity on solid ones."""
    T = u.dtype.type
    N = u.shape[0] - 2
    c_grad = T(0.5) * T(N)
    for b, x, xs, lo, hi in ((1, u, mk.vs[0], "ilo", "ihi"), (2, v, mk.vs[1], "jlo", "jhi"), (3, w, mk.vs[2], "klo", "khi")):
        val = x[I3] - c_grad * (mk.eff(p, hi) - mk.eff(p, lo))
        x[I3] = mk.zeroed(val) if mk.wrong == "solids_zero_after_project" else np.where(mk.solid, xs[I3], val)
        R.set_bnd(b, x)


def preconditioner(mask, m=0, mg=None, slabs=1):
    """z = M(r) as a whole field: mg = (nu, max_levels, nu_c) the masked V-cycle of §16, else m Jacobi sweeps of §11.2,
    else (m = 0) r itself, with which the loop below is §11's."""
    if mg:
        return lambda r: OM.vcycle(r, mask, *mg, slabs=slabs)
    if m > 0:
        return lambda r: Q.precondition(r, m)

    def identity(r):
        z = np.zeros(tuple(n + 2 for n in r.shape), r.dtype)
        z[I3] = r
        return z
    return identity


def project_cg(u, v, w, mask, vs, tol, max_iters, m=0, mg=None, slabs=1, wrong=None):
    """SPEC §19 project_cg on copies of u, v, w: §15's steps 2 to 4 verbatim (the loop of obstacles_mg_ref.project_cg
    with z = M(r) from preconditioner()), between the moving divergence and the moving gradient subtraction. Returns the
    dict of pressure_cg_ref.project_cg."""
    M = preconditioner(mask, m, mg, slabs)
    dtype = u.dtype
    T = dtype.type
    mk = Moving(mask, vs, wrong, slabs)
    u, v, w = u.copy(), v.copy(), w.copy()
    with np.errstate(all="ignore"):
        p, div = divergence(u, v, w, mk)
        s = R.tree_sum(div[I3].astype(np.float64), dtype, slabs)
        mu = T(s / float(mk.n_fluid)) if mk.n_fluid else T(0)
        r = np.where(mk.solid, T(0), div[I3] - mu)
        rho0 = last = R.dot(r, r, dtype, slabs)
        status, iters = MAX_ITERS, 0
        if rho0 == 0.0:
            status = CONVERGED
        elif not math.isfinite(rho0):
            status = BREAKDOWN
        else:
            z = M(r)
            gamma = R.dot(r, z[I3], dtype, slabs)
            if not gamma > 0.0:
                status = BREAKDOWN
            else:
                d = np.zeros_like(u)
                d[I3] = z[I3]
                R.set_bnd(0, d)
                for n in range(max_iters):
                    q = OB.apply_A(d, mk)
                    delta = R.dot(d[I3], q, dtype, slabs)
                    if not delta > 0.0:
                        status = BREAKDOWN
                        break
                    aT = T(gamma / delta)
                    p[I3] = p[I3] + aT * d[I3]
                    r = r - aT * q
                    rho_new = last = R.dot(r, r, dtype, slabs)
                    iters = n + 1
                    if not math.isfinite(rho_new):
                        status = BREAKDOWN
                        break
                    if rho_new <= (tol * tol) * rho0:
                        status = CONVERGED
                        break
                    z = M(r)
                    gamma_new = R.dot(r, z[I3], dtype, slabs)
                    if not gamma_new > 0.0:
                        status = BREAKDOWN
                        break
                    bT = T(gamma_new / gamma)
                    d[I3] = z[I3] + bT * d[I3]
                    R.set_bnd(0, d)
                    gamma = gamma_new
        R.set_bnd(0, p)
        subtract_gradient(u, v, w, p, mk)
        rel = 0.0 if rho0 == 0.0 else math.sqrt(last / rho0) if last / rho0 >= 0 else float("nan")
    return {"u": u, "v": v, "w": w, "p": p, "div": div, "status": status, "iterations": iters, "rel_residual": rel}


def sweep(b, x, x0, a, inv, mk):
    """The interior of one sweep of lin_solve_masked under a solid velocity: effv on the faces of axis b (b = 1, 2, 3),
    eff elsewhere; +0 on solid cells."""
    wrong = mk.wrong

    def e(face):
        if b != 0 and (AXIS[face] == b or wrong == "no_slip"):
            return mk.effv(x, face, b)
        if b == 0 and wrong == "effv_b0":
            return mk.effv(x, face)
        return mk.eff(x, face)

    with np.errstate(invalid="ignore", over="ignore"):
        val = (x0[I3] + a * (((e("ilo") + e("ihi")) + (e("jlo") + e("jhi"))) + (e("klo") + e("khi")))) * inv
    if wrong == "solids_set_by_sweep" and b != 0:
        return np.where(mk.solid, mk.vs[b - 1][I3], val)
    return mk.zeroed(val)


def lin_solve(b, x, x0, a, c, K, mask, vs, wrong=None, slabs=1):
    """§19 lin_solve_masked, in place in x (K = 0: a no-op)."""
    T = x.dtype.type
    mk = Moving(mask, vs, wrong, slabs)
    a, inv = T(a), T(1) / T(c)
    cur = x.copy()
    for _ in range(K):
        nxt = np.zeros_like(cur)
        nxt[I3] = sweep(b, cur, x0, a, inv, mk)
        S3.set_bnd(b, nxt)
        cur = nxt
    x[...] = cur


def diffuse(b, x, x0, diff, dt, K, mask, vs, wrong=None, slabs=1):
    T = x.dtype.type
    Nf = T(x.shape[0] - 2)
    a = ((T(dt) * T(diff)) * Nf) * Nf
    lin_solve(b, x, x0, a, T(1) + T(6) * a, K, mask, vs, wrong, slabs)


def advect(b, d, d0, u, v, w, dt, mask, vs, wrong=None, slabs=1):
    """§19 advect_masked: §17's with wv = xs_b[s], the solid velocity at the sample cell, for b = 1, 2, 3; b = 0 is
    §17's own."""
    if b == 0 and wrong != "effv_b0":
        TR.advect_masked(0, d, d0, u, v, w, dt, mask)
        return
    T = d.dtype.type
    N = d.shape[0] - 2
    mk = OB.Mask(mask)
    solid = OB.solid_cells(mask)
    xs = vs[(b if b else 1) - 1]
    if wrong == "wrong_axis":
        xs = vs[b % 3]
    dt0 = T(dt) * T(N)
    (i0, j0, k0), (x, y, z) = S3.SPEC.trace((u, v, w), dt0)
    kc = np.arange(1, N + 1).reshape(N, 1, 1)
    nzl = N // slabs
    with np.errstate(invalid="ignore", over="ignore"):
        s1, t1, r1 = x - i0.astype(T), y - j0.astype(T), z - k0.astype(T)
        s0, t0, r0 = T(1) - s1, T(1) - t1, T(1) - r1

        def at(di, dj, dk):
            ks, js = k0 + dk, j0 + dj
            val = d0[ks, js, i0 + di]
            sol = solid[ks, js, i0 + di]
            wv = xs[ks, js, i0 + (0 if wrong == "velocity_of_i0" else di)]
            if wrong == "wv_at_c":
                wv = xs[I3]
            if wrong == "xs_ghost_stale":  # the solid velocity across a slab boundary reads +0
                inner = (ks >= 1) & (ks <= N)
                wv = np.where(inner & ((ks - 1) // nzl != (kc - 1) // nzl), T(0), wv)
            if wrong == "fluid_entry":  # the select as a blend
                return val + sol.astype(T) * (wv - val)
            return np.where(sol, wv, val)

        def plane(di):
            return (t0 * (r0 * at(di, 0, 0) + r1 * at(di, 0, 1)) + t1 * (r0 * at(di, 1, 0) + r1 * at(di, 1, 1)))

        val = S3.SPEC.combine(s0, plane(0), s1, plane(1))
        d[I3] = np.where(mk.solid, xs[I3], val) if wrong == "solids_set_by_advect" else mk.zeroed(val)
    S3.set_bnd(b, d)


def vel_step(f, mask, vs, K, dt, visc, project, sources=None, forces=None, wrong=None):
    """§19 vel_step on copies of the velocity fields of f: §17's with the moving diffusions and advections.
    project(u, v, w): the moving projection in force (project_cg above with its settings). sources, forces: as in
    obstacle_transport_ref.vel_step. Returns the second projection's outcome."""
    u, v, w, u0, v0, w0 = (f[n].copy() for n in ("u", "v", "w", "u0", "v0", "w0"))
    if sources:
        u0, v0, w0 = (sources[n].copy() for n in ("u0", "v0", "w0"))
    if forces:
        F.add_forces(u, v, w, f["dens"], u0, v0, w0, **forces)
    for x, s in ((u, u0), (v, v0), (w, w0)):
        S3.add_source(x, s, dt)
    u, u0, v, v0, w, w0 = u0, u, v0, v, w0, w
    for b, x, x0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        diffuse(b, x, x0, visc, dt, K, mask, vs, wrong)
    out = project(u, v, w)
    u0, v0, w0 = out["u"], out["v"], out["w"]
    u, v, w = (np.zeros_like(u0) for _ in range(3))
    for b, d, d0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        advect(b, d, d0, u0, v0, w0, dt, mask, vs, wrong)
    return project(u, v, w)


dens_step = TR.dens_step  # §19 "Steps": dens_step is §17's exactly
