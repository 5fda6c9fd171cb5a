"""The CPU reference of docs/SPEC.md §8 (tests/forces_ref.py) against the closed forms of the SPEC, and against a
scalar cell-by-cell evaluation of the same expressions (which pins the reference's own expression order)."""
import numpy as np
import pytest

import forces_ref as F
from shape_cases import DTYPES

SIZES = [1, 2, 5, 17, 40]


def grid(N, dtype, fn):
    """fn(i, j, k) on every cell, shells included, evaluated in float64 and rounded to dtype."""
    k, j, i = np.meshgrid(*(np.arange(N + 2, dtype=np.float64),) * 3, indexing="ij")
    return np.asarray(fn(i, j, k), dtype=np.float64).astype(dtype) + np.zeros((N + 2,) * 3, dtype)


def force_inputs(N, dtype, seed):
    rng = np.random.RandomState(seed)
    return [rng.standard_normal((N + 2,) * 3).astype(dtype) for _ in range(7)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_uniform_velocity_gives_no_force(N, dtype):
    u = grid(N, dtype, lambda i, j, k: 0.75 + 0 * i)
    v = grid(N, dtype, lambda i, j, k: -1.5 + 0 * i)
    w = grid(N, dtype, lambda i, j, k: 3.0 + 0 * i)
    _, _, _, dens, su, sv, sw = force_inputs(N, dtype, 1)
    want = [a.copy() for a in (su, sv, sw)]
    F.add_forces(u, v, w, dens, su, sv, sw, eps=0.7)
    for got, ref in zip((su, sv, sw), want):
        assert np.array_equal(got, ref)
    assert not F.vorticity(u, v, w).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_rigid_rotation_gives_uniform_magnitude_and_no_force(N, dtype):
    c = N // 2
    u = grid(N, dtype, lambda i, j, k: -(j - c))
    v = grid(N, dtype, lambda i, j, k: i - c)
    w = grid(N, dtype, lambda i, j, k: 0 * i)
    mag = F.vorticity(u, v, w)
    # omega = (0, 0, c_grad * 4) = (0, 0, 2N) exactly; faces mirror it (the only shell cells confinement reads)
    assert (mag[1:-1, 1:-1, 1:-1] == dtype(2 * N)).all()
    for face in (mag[0, 1:-1, 1:-1], mag[-1, 1:-1, 1:-1], mag[1:-1, 0, 1:-1], mag[1:-1, -1, 1:-1],
                 mag[1:-1, 1:-1, 0], mag[1:-1, 1:-1, -1]):
        assert (face == dtype(2 * N)).all()
    _, _, _, dens, su, sv, sw = force_inputs(N, dtype, 2)
    want = [a.copy() for a in (su, sv, sw)]
    F.add_forces(u, v, w, dens, su, sv, sw, eps=0.4)
    for got, ref in zip((su, sv, sw), want):
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_shear_profile_closed_form(N, dtype):
    """u = w = 0, v = i^2: omega = (0, 0, 2 N i) exactly, n = (~1, 0, 0), f = (0, ~-2 eps i, 0). At N = 1 |omega| is
    uniform, so the gradient and the force vanish exactly."""
    eps = 0.3
    u = grid(N, dtype, lambda i, j, k: 0 * i)
    v = grid(N, dtype, lambda i, j, k: i * i)
    w = grid(N, dtype, lambda i, j, k: 0 * i)
    mag = F.vorticity(u, v, w)
    i_idx = np.arange(1, N + 1, dtype=np.float64)
    assert np.array_equal(mag[1:-1, 1:-1, 1:-1], np.broadcast_to((2.0 * N * i_idx).astype(dtype), (N, N, N)))
    z = np.zeros((N + 2,) * 3, dtype)
    su, sv, sw = z.copy(), z.copy(), z.copy()
    F.add_forces(u, v, w, z, su, sv, sw, eps=eps)
    assert not su.any() and not sw.any()
    assert not sv[0].any() and not sv[-1].any() and not sv[:, 0].any() and not sv[:, :, 0].any()
    fy = sv[1:-1, 1:-1, 1:-1].astype(np.longdouble)
    if N == 1:
        assert not fy.any()
        return
    want = np.broadcast_to(-2.0 * np.longdouble(eps) * i_idx.astype(np.longdouble), (N, N, N))
    tol = 8 * np.finfo(dtype).eps * np.abs(want)
    assert (np.abs(fy - want) <= tol).all(), float(np.max(np.abs(fy - want) / np.abs(want)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_buoyancy_on_uniform_density_is_one_rounding(N, dtype, axis):
    beta, C, amb = 0.37, 3.5, 0.5  # C - amb is exact: beta * 3 rounds once
    dens = grid(N, dtype, lambda i, j, k: C + 0 * i)
    u, v, w, _, su, sv, sw = force_inputs(N, dtype, 3)
    for a in (su, sv, sw):
        a[1:-1, 1:-1, 1:-1] = 0
    zeroed = [a.copy() for a in (su, sv, sw)]
    F.add_forces(u, v, w, dens, su, sv, sw, beta=beta, ambient=amb, axis=axis)
    fb = dtype(np.longdouble(dtype(beta)) * (np.longdouble(C) - np.longdouble(amb)))
    for a, (got, ref) in enumerate(zip((su, sv, sw), zeroed)):
        if a == axis:
            assert (got[1:-1, 1:-1, 1:-1] == fb).all()
            ref = ref.copy()
            ref[1:-1, 1:-1, 1:-1] = fb
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_zero_coefficients_evaluate_nothing(dtype):
    N = 5
    u, v, w, dens, su, sv, sw = force_inputs(N, dtype, 4)
    sv[2, 2, 2] = -0.0
    u[1, 1, 1] = np.nan
    want = [a.copy() for a in (su, sv, sw)]
    F.add_forces(u, v, w, dens, su, sv, sw, eps=0.0, beta=0.0)
    for got, ref in zip((su, sv, sw), want):
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8))


def scalar_force(u, v, w, dens, s, k, j, i, eps, beta, amb, axis):
    """SPEC §8 add_forces at one cell with numpy scalars of the arrays' dtype: the expressions written out."""
    T = u.dtype.type
    N = u.shape[0] - 2
    Nf = T(N)
    h = T(1) / Nf
    cg = T(0.5) * Nf
    eps_h = T(eps) * h

    def om(k, j, i):
        wx = cg * ((w[k, j + 1, i] - w[k, j - 1, i]) - (v[k + 1, j, i] - v[k - 1, j, i]))
        wy = cg * ((u[k + 1, j, i] - u[k - 1, j, i]) - (w[k, j, i + 1] - w[k, j, i - 1]))
        wz = cg * ((v[k, j, i + 1] - v[k, j, i - 1]) - (u[k, j + 1, i] - u[k, j - 1, i]))
        return wx, wy, wz

    def mag(k, j, i):  # a face cell holds the value of its interior neighbour (set_bnd(0): T(1) * x)
        k, j, i = (min(max(a, 1), N) for a in (k, j, i))
        wx, wy, wz = om(k, j, i)
        return np.sqrt((wx * wx + wy * wy) + wz * wz)

    wx, wy, wz = om(k, j, i)
    ex = cg * (mag(k, j, i + 1) - mag(k, j, i - 1))
    ey = cg * (mag(k, j + 1, i) - mag(k, j - 1, i))
    ez = cg * (mag(k + 1, j, i) - mag(k - 1, j, i))
    ln = np.sqrt((ex * ex + ey * ey) + ez * ez)
    r = T(1) / (ln + T(1e-20))
    nx, ny, nz = ex * r, ey * r, ez * r
    out = [s[0][k, j, i], s[1][k, j, i], s[2][k, j, i]]
    out[0] = out[0] + eps_h * ((ny * wz) - (nz * wy))
    out[1] = out[1] + eps_h * ((nz * wx) - (nx * wz))
    out[2] = out[2] + eps_h * ((nx * wy) - (ny * wx))
    out[axis] = out[axis] + T(beta) * (dens[k, j, i] - T(amb))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_vectorised_reference_equals_scalar_evaluation(dtype):
    N, eps, beta, amb, axis = 17, 0.45, -1.3, 0.2, 2
    u, v, w, dens, su, sv, sw = force_inputs(N, dtype, 5)
    src = [a.copy() for a in (su, sv, sw)]
    F.add_forces(u, v, w, dens, su, sv, sw, eps=eps, beta=beta, ambient=amb, axis=axis)
    rng = np.random.RandomState(6)
    cells = rng.randint(1, N + 1, size=(200, 3))
    cells[:20, 2] = 1  # next to the shells, where mag is read from the faces
    cells[20:40, 0] = N
    with np.errstate(all="ignore"):
        for k, j, i in cells:
            want = scalar_force(u, v, w, dens, src, k, j, i, eps, beta, amb, axis)
            for a, got in enumerate((su, sv, sw)):
                assert got[k, j, i].tobytes() == want[a].tobytes(), (k, j, i, a, got[k, j, i], want[a])
            assert isinstance(want[0], dtype)
