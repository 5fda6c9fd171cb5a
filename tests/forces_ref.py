"""CPU reference of docs/SPEC.md §8 (external forces: vorticity confinement and buoyancy) in numpy.

Arrays are (N+2,)*3 indexed [k, j, i], in the context's dtype (float32 / float64). Every scalar is rounded to that
dtype first and every operation below is one numpy operation on that dtype, in the SPEC's bracketing: numpy rounds
each one (no contraction), and its sqrt and division are correctly rounded. set_bnd is the oracle's (SPEC §3).
The full step with forces is `add_forces(...)` followed by `oracle_lib.vel_step` and `oracle_lib.dens_step`."""
import numpy as np

import oracle_lib as O

I, P, M = slice(1, -1), slice(2, None), slice(None, -2)


def scalars(N, dtype, eps=0.0, beta=0.0, ambient=0.0):
    T = np.dtype(dtype).type
    Nf = T(N)
    h = T(1) / Nf
    return {"c_grad": T(0.5) * Nf, "eps_h": T(eps) * h, "eps": T(eps), "beta": T(beta), "amb": T(ambient),
            "tiny": T(1e-20)}


def curl(u, v, w, c_grad):
    """(wx, wy, wz) on the interior cells, shells of u, v, w read as stored."""
    wx = c_grad * ((w[I, P, I] - w[I, M, I]) - (v[P, I, I] - v[M, I, I]))
    wy = c_grad * ((u[P, I, I] - u[M, I, I]) - (w[I, I, P] - w[I, I, M]))
    wz = c_grad * ((v[I, I, P] - v[I, I, M]) - (u[I, P, I] - u[I, M, I]))
    return wx, wy, wz


def vorticity(u, v, w):
    """SPEC §8 vorticity: |omega| on the interior, then set_bnd(0) (faces, edges, corners)."""
    N = u.shape[0] - 2
    s = scalars(N, u.dtype)
    wx, wy, wz = curl(u, v, w, s["c_grad"])
    mag = np.zeros_like(u)
    mag[I, I, I] = np.sqrt((wx * wx + wy * wy) + wz * wz)
    O.set_bnd(0, mag)
    return mag


def confinement(u, v, w):
    """SPEC §8 confinement force (fx, fy, fz) on the interior cells, without the factor eps_h."""
    N = u.shape[0] - 2
    s = scalars(N, u.dtype)
    cg = s["c_grad"]
    mag = vorticity(u, v, w)
    wx, wy, wz = curl(u, v, w, cg)
    ex = cg * (mag[I, I, P] - mag[I, I, M])
    ey = cg * (mag[I, P, I] - mag[I, M, I])
    ez = cg * (mag[P, I, I] - mag[M, I, I])
    ln = np.sqrt((ex * ex + ey * ey) + ez * ez)
    r = u.dtype.type(1) / (ln + s["tiny"])
    nx, ny, nz = ex * r, ey * r, ez * r
    return (ny * wz) - (nz * wy), (nz * wx) - (nx * wz), (nx * wy) - (ny * wx)


def add_forces(u, v, w, dens, su, sv, sw, eps=0.0, beta=0.0, ambient=0.0, axis=1):
    """SPEC §8 add_forces: su, sv, sw (modified in place) += the forces on interior cells; shells untouched. A term
    whose coefficient is zero (in the dtype) is not evaluated."""
    N = u.shape[0] - 2
    s = scalars(N, u.dtype, eps, beta, ambient)
    src = (su, sv, sw)
    if s["eps"] != 0:
        f = confinement(u, v, w)
        for a in range(3):
            src[a][I, I, I] = src[a][I, I, I] + s["eps_h"] * f[a]
    if s["beta"] != 0:
        fb = s["beta"] * (dens[I, I, I] - s["amb"])
        src[axis][I, I, I] = src[axis][I, I, I] + fb


def step(fields, dt, diff, visc, K, eps=0.0, beta=0.0, ambient=0.0, axis=1, bound=None):
    """vel_step with forces, then dens_step, on a dict of the 8 named fields (in place; returned). `bound`: a dict
    {"u0": array, ...} of bound sources, copied into the x0 slots first (sf_bind_sources)."""
    f = fields
    T = f["u"].dtype.type
    if bound:
        for n, a in bound.items():
            f[n][...] = a
    add_forces(f["u"], f["v"], f["w"], f["dens"], f["u0"], f["v0"], f["w0"], eps, beta, ambient, axis)
    O.vel_step(f["u"], f["v"], f["w"], f["u0"], f["v0"], f["w0"], T(visc), T(dt), K)
    O.dens_step(f["dens"], f["dens0"], f["u"], f["v"], f["w"], T(diff), T(dt), K)
    return f
