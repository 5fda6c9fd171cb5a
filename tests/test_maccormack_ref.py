"""The CPU reference of docs/SPEC.md §9 (tests/maccormack_ref.py) against the closed forms of §9.1, against a scalar
cell-by-cell evaluation of the same expressions, on the translating-bump experiment that motivates the scheme, and —
with both schemes first-order — against the oracle's own step."""
import numpy as np
import pytest

import maccormack_ref as M
import oracle_lib as O
from gpu_support import DTYPES, NAMES

I = M.I


def rand(N, dtype, seed, scale=1.0):
    return (scale * np.random.RandomState(seed).standard_normal((N + 2,) * 3)).astype(dtype)


def mc(b, d0, u, v, w, dt):
    return M.advect_mc(b, np.zeros_like(d0), d0, u, v, w, dt)


# ---- §9.1 closed forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", [1, 2, 5, 17])
@pytest.mark.parametrize("b", [0, 1, 2, 3])
def test_zero_velocity_is_the_identity_in_value(N, b, dtype):
    d0 = rand(N, dtype, 1 + N)
    d0[2 % (N + 2), 1, 1] = dtype(-0.0)  # a -0 may come back as +0: equal in value
    O.set_bnd(b, d0)
    z = np.zeros_like(d0)
    assert np.array_equal(mc(b, d0, z, z, z, 0.1), d0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,sigma", [(12, 0.2), (17, 1.0), (24, 3.0)])
def test_every_cell_is_bounded_or_first_order(N, sigma, dtype):
    d0 = rand(N, dtype, 3)
    u, v, w = (rand(N, dtype, 4 + q, sigma) for q in range(3))
    dt = 0.1
    d = mc(0, d0, u, v, w, dt)
    p = M.parts(0, d0, u, v, w, dt)
    inside = (d[I] >= p["mn"]) & (d[I] <= p["mx"])
    assert (inside | (d[I] == p["hat"][I])).all()
    assert d[I].max() <= d0.max() and d[I].min() >= d0.min()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,U", [(16, (0.3, -0.45, 0.2)), (20, (-0.7, 0.1, 0.55)), (12, (2.6, -1.3, 0.4))])
def test_affine_field_in_uniform_flow(N, U, dtype):
    """d = alpha + beta.((i,j,k) - dt*N*U) within 32 eps max|d0| wherever neither trace is clamped and the reverse
    trace reads no shell cell of hat (set_bnd makes hat's shell a mirror image, which is not affine)."""
    dt = 0.1
    al, be = 0.5, (0.25, -0.75, 1.5)
    k, j, i = np.meshgrid(*(np.arange(N + 2, dtype=np.float64),) * 3, indexing="ij")
    d0 = (al + be[0] * i + be[1] * j + be[2] * k).astype(dtype)
    vel = [np.full_like(d0, c / (dt * N)) for c in U]
    d = mc(0, d0, *vel, dt)
    p = M.parts(0, d0, *vel, dt)
    rev, _ = M.trace(vel, dtype(dt) * dtype(N), +1)
    free = ~(p["cf"] | p["cr"])
    # (shifts below half a cell clamp nothing; larger ones clamp the cells next to a wall)
    assert free.any() and free.all() == (max(abs(c) for c in U) <= 0.5)
    for r0 in rev:
        free &= (r0 >= 1) & (r0 + 1 <= N)
    assert free.mean() > 0.3
    shift = [float(dtype(dt) * dtype(N)) * float(c[0, 0, 0]) for c in vel]
    want = al + be[0] * (i - shift[0]) + be[1] * (j - shift[1]) + be[2] * (k - shift[2])
    tol = 32 * np.finfo(dtype).eps * float(np.abs(d0).max())
    assert np.abs(d[I].astype(np.float64) - want[I])[free].max() <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("b", [0, 1, 2, 3])
def test_cells_whose_trace_touched_a_wall_equal_advect(b, dtype):
    N, dt = 14, 0.1
    d0 = rand(N, dtype, 7)
    u, v, w = (rand(N, dtype, 8 + q, 1.5) for q in range(3))
    d = mc(b, d0, u, v, w, dt)
    hat = np.zeros_like(d0)
    O.advect(b, hat, d0, u, v, w, dtype(dt))
    _, cf = M.trace((u, v, w), dtype(dt) * dtype(N), -1)
    _, cr = M.trace((u, v, w), dtype(dt) * dtype(N), +1)
    wall = cf | cr
    assert 0.05 < wall.mean() < 0.95
    assert np.array_equal(d[I][wall].view(np.uint8), hat[I][wall].view(np.uint8))
    assert (d[I][~wall] != hat[I][~wall]).any()


# ---- the vectorised reference against a scalar evaluation ----------------------------------------------------------
def scalar_cell(T, N, b, d0, hat, u, v, w, dt, i, j, k):
    """SPEC §9 step 2 for one interior cell in scalar arithmetic on the dtype (hat given)."""
    dt0 = T(dt) * T(N)
    lo, hi = T(0.5), T(N) + T(0.5)

    def tr(sign):
        pos, idx, clamped = [], [], False
        for c, vel in ((i, u), (j, v), (k, w)):
            a = dt0 * vel[k, j, i]
            x = T(c) - a if sign < 0 else T(c) + a
            if x < lo:
                x, clamped = lo, True
            if x > hi:
                x, clamped = hi, True
            pos.append(x)
            idx.append(int(x))
        return pos, idx, clamped

    _, (i0, j0, k0), cf = tr(-1)
    (x, y, z), (ir, jr, kr), cr = tr(+1)
    s1, t1, r1 = x - T(ir), y - T(jr), z - T(kr)
    s0, t0, r0 = T(1) - s1, T(1) - t1, T(1) - r1
    h = lambda a, c, e: hat[kr + e, jr + c, ir + a]
    bar = (s0 * (t0 * (r0 * h(0, 0, 0) + r1 * h(0, 0, 1)) + t1 * (r0 * h(0, 1, 0) + r1 * h(0, 1, 1))) +
           s1 * (t0 * (r0 * h(1, 0, 0) + r1 * h(1, 0, 1)) + t1 * (r0 * h(1, 1, 0) + r1 * h(1, 1, 1))))
    a = lambda p, q, r: d0[k0 + r, j0 + q, i0 + p]
    mn_ = lambda p, q: q if q < p else p
    mx_ = lambda p, q: q if q > p else p
    mn = mn_(mn_(mn_(a(0, 0, 0), a(0, 0, 1)), mn_(a(0, 1, 0), a(0, 1, 1))),
             mn_(mn_(a(1, 0, 0), a(1, 0, 1)), mn_(a(1, 1, 0), a(1, 1, 1))))
    mx = mx_(mx_(mx_(a(0, 0, 0), a(0, 0, 1)), mx_(a(0, 1, 0), a(0, 1, 1))),
             mx_(mx_(a(1, 0, 0), a(1, 0, 1)), mx_(a(1, 1, 0), a(1, 1, 1))))
    r = hat[k, j, i] + T(0.5) * (d0[k, j, i] - bar)
    if r < mn:
        r = mn
    if r > mx:
        r = mx
    if cf or cr:
        r = hat[k, j, i]
    return r, (cf or cr)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_vectorised_reference_equals_scalar_evaluation(dtype):
    N, dt, b = 9, 0.1, 2
    d0 = rand(N, dtype, 21)
    u, v, w = (rand(N, dtype, 22 + q, 0.6) for q in range(3))
    d = mc(b, d0, u, v, w, dt)
    hat = np.zeros_like(d0)
    O.advect(b, hat, d0, u, v, w, dtype(dt))
    seen = set()
    for k in range(1, N + 1):
        for j in range(1, N + 1):
            for i in range(1, N + 1):
                r, wall = scalar_cell(dtype, N, b, d0, hat, u, v, w, dt, i, j, k)
                seen.add(bool(wall))
                assert r.dtype == np.dtype(dtype) and r.tobytes() == d[k, j, i].tobytes(), (i, j, k, r, d[k, j, i])
    assert seen == {False, True}  # at least one interior and one wall cell went through the scalar form
    # shells: the oracle's set_bnd of the interior
    want = d.copy()
    O.set_bnd(b, want)
    assert np.array_equal(want, d)


# ---- the experiment that motivates the scheme -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_translating_bump_keeps_its_shape(dtype):
    """A Gaussian bump (sigma = 4 cells, N = 48) carried 14.8 x 8.4 cells in 40 steps by a uniform flow. Measured: RMS
    error ratio advect / MacCormack 4.30, peaks 0.665 / 0.962, in both precisions."""
    N, dt, steps = 48, 0.1, 40
    k, j, i = np.meshgrid(*(np.arange(N + 2, dtype=np.float64),) * 3, indexing="ij")
    cells = (0.37, 0.21)  # per step along i and j
    u = np.full((N + 2,) * 3, cells[0] / (dt * N), dtype)
    v = np.full((N + 2,) * 3, cells[1] / (dt * N), dtype)
    w = np.zeros((N + 2,) * 3, dtype)

    def bump(ci, cj):
        return np.exp(-((i - ci) ** 2 + (j - cj) ** 2 + (k - N / 2) ** 2) / (2 * 4.0 ** 2))

    sl = bump(14.0, 16.0).astype(dtype)
    m = sl.copy()
    for _ in range(steps):
        nxt = np.zeros_like(sl)
        O.advect(0, nxt, sl, u, v, w, dtype(dt))
        sl = nxt
        m = mc(0, m, u, v, w, dt)
    exact = bump(14.0 + cells[0] * steps, 16.0 + cells[1] * steps)
    rms = lambda a: float(np.sqrt(np.mean((a[I].astype(np.float64) - exact[I]) ** 2)))
    print(f"bump {np.dtype(dtype).name}: rms advect {rms(sl):.5f} maccormack {rms(m):.5f} ratio {rms(sl) / rms(m):.2f} "
          f"peaks {float(sl.max()):.3f} {float(m.max()):.3f}")
    assert rms(sl) / rms(m) >= 3
    assert float(m.max()) >= 0.9
    assert float(sl.max()) <= 0.7


# ---- step() ------------------------------------------------------------------------------------------------------


def fields(N, dtype, seed):
    rng = np.random.RandomState(seed)
    return {n: (0.2 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in NAMES}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,K", [(8, 0), (12, 3), (17, 6)])
def test_first_order_step_equals_the_oracle_step(N, K, dtype):
    f = fields(N, dtype, 30 + N)
    want = {n: a.copy() for n, a in f.items()}
    for _ in range(2):
        M.step(f, 0.1, 1e-4, 1e-4, K)
        O.step(N, want, 0.1, 1e-4, 1e-4, K)
    for n in NAMES:
        assert np.array_equal(f[n].view(np.uint8), want[n].view(np.uint8)), n


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_each_scheme_changes_only_its_own_step(dtype):
    N, K = 12, 3
    base = M.step(fields(N, dtype, 5), 0.1, 1e-4, 1e-4, K)
    vel = M.step(fields(N, dtype, 5), 0.1, 1e-4, 1e-4, K, velocity=M.MACCORMACK)
    dens = M.step(fields(N, dtype, 5), 0.1, 1e-4, 1e-4, K, density=M.MACCORMACK)
    assert not np.array_equal(vel["u"], base["u"])
    assert np.array_equal(dens["u"], base["u"]) and not np.array_equal(dens["dens"], base["dens"])
