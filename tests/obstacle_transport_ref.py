"""numpy reference of docs/SPEC.md §17 "Mask-aware transport", written from the SPEC text on the pieces of
tests/obstacles_ref.py (Mask, eff / effn, solid_cells) and tests/stable_ref.py (set_bnd, add_source, the back-trace of
advect). It does not call the library. Fields and the mask are (N+2, N+2, N+2) arrays indexed [k, j, i]; every per-cell
expression is one numpy operation per SPEC operation on the dtype, every face, sample and solid rule a select (np.where)
on values that are all evaluated.

`wrong` names one deliberately wrong reading of §17 (WRONG): tests/test_obstacle_transport_ref.py shows for each of them
a case whose result it changes, so that a test against this reference tells that reading from the SPEC's.
"""
import numpy as np

import forces_ref as F
import obstacles_ref as OB
import stable_ref as S3

I = (slice(1, -1),) * 3
AXIS = {"ilo": 1, "ihi": 1, "jlo": 2, "jhi": 2, "klo": 3, "khi": 3}
WRONG = ("closed_stored", "eff_everywhere", "no_slip", "solids_not_zeroed", "sample_stored", "wv_zero_b0", "wv_own_bn",
         "solidity_of_i0", "shell_solid", "code_ghost_stale", "dens_zero_solid")
# Wrong readings that only special values in the fluid tell from §17 (tests/test_obstacle_special_inputs_ref.py): two
# names for `wrong`, and four stable_ref.Ops for `ops`: plausible rewrites of a masked kernel's arithmetic, the same
# ones tests/test_stable_inputs_ref.py holds the unmasked §3 operators against.
SPECIAL_WRONG = ("solid_as_product", "replace_as_blend")


def flush(x):
    """Subnormals to a zero of the same sign."""
    return np.where(np.abs(x) < np.finfo(x.dtype).tiny, x.dtype.type(0) * x, x)


def hw_clamp(x, lo, hi):
    return np.fmax(lo, np.fmin(hi, x))  # a hardware min / max: a NaN operand is ignored


class ClampMinMax(S3.Ops):  # the advect clamps as fmax(lo, fmin(hi, x))
    def trace(self, vel, dt0):
        T = vel[0].dtype.type
        N = vel[0].shape[0] - 2
        idx, pos = [], []
        for ax, comp in enumerate(vel):
            shape = [1, 1, 1]
            shape[2 - ax] = N
            with np.errstate(invalid="ignore"):
                x = hw_clamp(np.arange(1, N + 1).astype(T).reshape(shape) - dt0 * comp[I], T(0.5), T(N) + T(0.5))
            idx.append(np.clip(x.astype(np.int64), 0, N))
            pos.append(x)
        return idx, pos


class Flush(S3.Ops):  # subnormals flushed to zero on the way in and out of a masked sweep
    def sweep_io(self, x):
        return flush(x)


class FaceMinus(S3.Ops):  # effn as T(0) - x
    def neg(self, x):
        return x.dtype.type(0) - x


class SkipZeroWeight(S3.Ops):  # advect skips the i0 + 1 samples where s1 == 0
    def combine(self, s0, lo, s1, hi):
        return np.where(s1 == 0, s0 * lo, s0 * lo + s1 * hi)


MUTANTS = (ClampMinMax, Flush, FaceMinus, SkipZeroWeight)


def sweep_masked(b, x, x0, a, inv, mk, wrong=None, ops=S3.SPEC):
    """The interior of one sweep of lin_solve_masked: the neighbour operand of a face on axis A is effn when b == A and
    eff otherwise; +0 on solid cells."""
    x, x0 = ops.sweep_io(x), ops.sweep_io(x0)

    def e(face):
        if wrong == "closed_stored":
            return x[dict(OB.FACES)[face]]
        sign = -1 if b == AXIS[face] else 1
        if wrong == "eff_everywhere":
            sign = 1
        if wrong == "no_slip" and b != 0:
            sign = -1
        return mk.eff(x, face, sign, ops)

    with np.errstate(invalid="ignore", over="ignore"):
        val = (x0[I] + a * (((e("ilo") + e("ihi")) + (e("jlo") + e("jhi"))) + (e("klo") + e("khi")))) * inv
    return val if wrong == "solids_not_zeroed" else mk.zeroed(ops.sweep_io(val), wrong)


def lin_solve_masked(b, x, x0, a, c, K, mask, wrong=None, ops=S3.SPEC):
    """§17 lin_solve_masked, in place in x (K = 0: a no-op)."""
    T = x.dtype.type
    mk = OB.Mask(mask)
    a, inv = T(a), T(1) / T(c)
    cur = x.copy()
    for _ in range(K):
        nxt = np.zeros_like(cur)
        nxt[I] = sweep_masked(b, cur, x0, a, inv, mk, wrong, ops)
        S3.set_bnd(b, nxt)
        cur = nxt
    x[...] = cur


def diffuse_masked(b, x, x0, diff, dt, K, mask, wrong=None, ops=S3.SPEC):
    T = x.dtype.type
    Nf = T(x.shape[0] - 2)
    a = ((T(dt) * T(diff)) * Nf) * Nf
    lin_solve_masked(b, x, x0, a, T(1) + T(6) * a, K, mask, wrong, ops)


def advect_masked(b, d, d0, u, v, w, dt, mask, wrong=None, slabs=1, ops=S3.SPEC):
    """§17 advect_masked: §3's advect with each sample solid(s) ? wv : d0[s], +0 on solid cells, set_bnd(b, d).
    slabs (wrong "code_ghost_stale" only): the k-slabs whose codes a stale ghost plane hides from each other."""
    T = d.dtype.type
    N = d.shape[0] - 2
    mk = OB.Mask(mask)
    solid = OB.solid_cells(mask)  # (N+2)^3: shell cells are never solid
    if wrong == "shell_solid":
        with np.errstate(invalid="ignore"):
            solid = mask > 0
    dt0 = T(dt) * T(N)
    (i0, j0, k0), (x, y, z) = ops.trace((u, v, w), dt0)
    own = d0[I]
    carries = b == 0  # wv = d0[c] for b = 0, T(0) for a velocity component
    if wrong == "wv_zero_b0" and b == 0:
        carries = False
    if wrong == "wv_own_bn" and b != 0:
        carries = True
    wv = own if carries else np.zeros_like(own)
    kc = np.arange(1, N + 1).reshape(N, 1, 1)
    nzl = N // slabs
    with np.errstate(invalid="ignore", over="ignore"):
        s1, t1, r1 = x - i0.astype(T), y - j0.astype(T), z - k0.astype(T)
        s0, t0, r0 = T(1) - s1, T(1) - t1, T(1) - r1

        def at(di, dj, dk):
            ks, js = k0 + dk, j0 + dj
            val = d0[ks, js, i0 + di]
            sol = solid[ks, js, i0 + (0 if wrong == "solidity_of_i0" else di)]
            if wrong == "code_ghost_stale":  # the code across a slab boundary reads as fluid
                inner = (ks >= 1) & (ks <= N)
                sol = sol & ~(inner & ((ks - 1) // nzl != (kc - 1) // nzl))
            if wrong == "replace_as_blend":  # val + s (wv - val) with s = 1 on a solid sample, 0 on a fluid one
                return val + sol.astype(T) * (wv - val)
            return val if wrong == "sample_stored" else np.where(sol, wv, val)

        def plane(di):
            return (t0 * (r0 * at(di, 0, 0) + r1 * at(di, 0, 1)) + t1 * (r0 * at(di, 1, 0) + r1 * at(di, 1, 1)))

        val = ops.combine(s0, plane(0), s1, plane(1))
        d[I] = mk.zeroed(val, wrong)
    S3.set_bnd(b, d)


def vel_step(f, mask, K, dt, visc, project, sources=None, forces=None, wrong=None, ops=S3.SPEC):
    """§17 vel_step on copies of the velocity fields of f. project(u, v, w): the masked projection in force, returning
    the dict of obstacles_ref.project_cg. sources: bound sources, copied into the x0 fields first; forces: the keywords
    of forces_ref.add_forces (SPEC §8; reads f["dens"]). Returns the second projection's outcome."""
    u, v, w, u0, v0, w0 = (f[n].copy() for n in ("u", "v", "w", "u0", "v0", "w0"))
    if sources:
        u0, v0, w0 = (sources[n].copy() for n in ("u0", "v0", "w0"))
    if forces:
        F.add_forces(u, v, w, f["dens"], u0, v0, w0, **forces)
    for x, s in ((u, u0), (v, v0), (w, w0)):
        S3.add_source(x, s, dt)
    u, u0, v, v0, w, w0 = u0, u, v0, v, w0, w
    for b, x, x0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        diffuse_masked(b, x, x0, visc, dt, K, mask, wrong, ops)
    out = project(u, v, w)
    u0, v0, w0 = out["u"], out["v"], out["w"]
    u, v, w = (np.zeros_like(u0) for _ in range(3))
    for b, d, d0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        advect_masked(b, d, d0, u0, v0, w0, dt, mask, wrong, ops=ops)
    return project(u, v, w)


def dens_step(dens, dens0, u, v, w, mask, K, dt, diff, source=None, wrong=None, ops=S3.SPEC):
    """§17 dens_step on copies: add_source, diffuse_masked(0), advect_masked(0); no zero_solid. Returns the density."""
    x, x0 = dens.copy(), (source if source is not None else dens0).copy()
    S3.add_source(x, x0, dt)
    x, x0 = x0, x
    diffuse_masked(0, x, x0, diff, dt, K, mask, wrong, ops)
    x, x0 = x0, x
    if wrong == "dens_zero_solid":  # §15's end of the step kept: the unmasked advect, then the solids zeroed
        S3.advect(0, x, x0, u, v, w, dt)
        return OB.zero_solids(x, mask)
    advect_masked(0, x, x0, u, v, w, dt, mask, wrong, ops=ops)
    return x
