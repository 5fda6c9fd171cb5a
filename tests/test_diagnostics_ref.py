"""Closed forms of the numpy reference of docs/SPEC.md §10 (tests/diagnostics_ref.py). No GPU needed: this pins the
reference the GPU results are compared with bit for bit (tests/test_diagnostics_gpu.py)."""
import math

import numpy as np
import pytest

import diagnostics_ref as D
from shape_cases import DT, DTYPES

SIZES = [1, 2, 5, 17, 64, 70]  # tails, non-multiples of W, non-powers of two, more than one vector per lane (70: fp64)


def divisors(N):
    return [p for p in range(1, N + 1) if N % p == 0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_constant_field_is_exact(N, dtype):
    for C in (3, -7):
        x = np.full((N + 2,) * 3, C, dtype)
        x[0] = 1e30  # shell cells are never counted
        x[:, :, -1] = np.nan
        assert D.reduce("sum", x) == C * N ** 3
        assert D.reduce("sum_sq", x) == C * C * N ** 3
        assert D.reduce("min", x) == C and D.reduce("max", x) == C
        assert D.reduce("max_abs", x) == abs(C)
        assert D.reduce("count_nonfinite", x) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_sum_within_the_tree_bound(N, dtype):
    """|SUM - fsum| <= (additions on the longest path of the tree) * 2^-53 * sum|x|: every addition on the path from
    a cell to the total rounds once, with relative error at most the unit roundoff 2^-53 of a double, and the partial
    sums it rounds are bounded by sum|x|. A bound derived from the tree, not a measurement."""
    rng = np.random.RandomState(N)
    x = (rng.standard_normal((N + 2,) * 3) * 10.0 ** rng.randint(-3, 4, (N + 2,) * 3)).astype(dtype)
    inner = x[1:-1, 1:-1, 1:-1].astype(np.float64).ravel()
    path = D.sum_path_additions(N, dtype)
    assert path >= N
    bound = path * 2.0 ** -53 * math.fsum(np.abs(inner))
    err = abs(D.reduce("sum", x) - math.fsum(inner))
    print(f"N={N} {np.dtype(dtype).name}: path {path} err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    sq = abs(D.reduce("sum_sq", x) - math.fsum(inner * inner))
    # the squares of fp32 values are exact in double; those of fp64 values round once (one more 2^-53 each)
    assert sq <= (path + 1) * 2.0 ** -53 * math.fsum(inner * inner)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_nonfinite_cells_are_skipped_and_counted(N, dtype):
    rng = np.random.RandomState(7 + N)
    x = rng.standard_normal((N + 2,) * 3).astype(dtype)
    y = x.copy()
    cells = {(1, 1, 1), (N, N, N), (N, 1, (N + 1) // 2)}
    for n, (k, j, i) in enumerate(sorted(cells)):
        y[k, j, i] = (np.nan, np.inf, -np.inf)[n % 3]
    inner = y[1:-1, 1:-1, 1:-1]
    fin = inner[np.isfinite(inner)].astype(np.float64)
    want = {"min": fin.min() if fin.size else np.inf, "max": fin.max() if fin.size else -np.inf,
            "max_abs": np.abs(fin).max() if fin.size else 0.0}
    for op, val in want.items():
        assert D.bits(D.reduce(op, y)) == D.bits(float(val) + 0.0), op
    assert D.reduce("count_nonfinite", y) == len(cells)
    # no finite candidate: the starting value comes back
    z = np.full((N + 2,) * 3, np.nan, dtype)
    z[1, 1, 1] = np.inf
    assert D.reduce("min", z) == np.inf and D.reduce("max", z) == -np.inf
    assert D.bits(D.reduce("max_abs", z)) == D.bits(0.0)
    assert D.reduce("count_nonfinite", z) == N ** 3


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_negative_zero_gives_positive_zero(N, dtype):
    x = np.full((N + 2,) * 3, -0.0, dtype)
    for op in D.OPS:
        assert D.bits(D.reduce(op, x)) == D.bits(0.0), op
    d = D.diagnostics(x, x, x, x, DT)
    for name, val in d.items():
        assert D.bits(val) == D.bits(0.0) if name != "nonfinite" else val == 0, name


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_every_slab_count_gives_the_same_bits(N, dtype):
    rng = np.random.RandomState(11 + N)
    f = [rng.standard_normal((N + 2,) * 3).astype(dtype) for _ in range(4)]
    f[0][1, 1, 1] = np.nan
    f[3][N, N, N] = np.inf
    one = {op: D.bits(D.reduce(op, f[1])) for op in D.OPS}
    one_nan = {op: D.bits(D.reduce(op, f[0])) for op in D.OPS}
    d1 = D.diagnostics(*f, DT)
    for P in divisors(N):
        for op in D.OPS:
            assert D.bits(D.reduce_slabs(op, f[1], P)) == one[op], (op, P)
            assert D.bits(D.reduce_slabs(op, f[0], P)) == one_nan[op], (op, P)
        dP = D.diagnostics(*f, DT, P=P)
        assert {k: D.bits(v) for k, v in dP.items()} == {k: D.bits(v) for k, v in d1.items()}, P
    assert d1["nonfinite"] == (2 if N > 1 else 1)


def mode(N, mx, my, mz, kinds):
    """Product of psi (antisymmetric, 's') / phi (symmetric, 'c') modes of SPEC §7.1 on all N + 2 indices, [k, j, i]."""
    i = np.arange(N + 2, dtype=np.float64)
    fx, fy, fz = ((np.sin if kind == "s" else np.cos)(np.pi * m * (i - 0.5) / N) for kind, m in zip(kinds, (mx, my, mz)))
    return fz[:, None, None] * fy[None, :, None] * fx[None, None, :]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", [5, 17, 64, 70])
def test_divergence_free_mode_pair(N, dtype):
    """u = U psi phi phi, v = V phi psi phi with U s_x + V s_y = 0 (SPEC §7.1): div = 0 in exact arithmetic.
    Bound on what the six operations of the expression leave, with unit roundoff r = eps/2 and amplitude A <= 1:
    each of the four non-zero inputs carries at most 16 r A (rounding to T, the three sin / cos evaluations and their
    argument, the products that build it): 64 r A; the two non-zero differences (|.| <= 2A) round once each: 4 r A;
    the two additions, of magnitude <= 4A: 8 r A; w's difference is exact (0) and the product by c_div adds a factor
    (1 + r). Together < 80 r A |c_div| = 40 eps A |c_div|."""
    mx, my, mz = 1, 2, 1
    sx, sy = math.sin(math.pi * mx / N), math.sin(math.pi * my / N)
    U, V = sy, -sx
    u = (U * mode(N, mx, my, mz, "scc")).astype(dtype)
    v = (V * mode(N, mx, my, mz, "csc")).astype(dtype)
    w = np.zeros_like(u)
    d = D.diagnostics(u, v, w, np.ones_like(u), DT)
    A = max(abs(U), abs(V))
    bound = 40 * np.finfo(dtype).eps * A * 0.5 / N
    print(f"N={N} {np.dtype(dtype).name}: max_div {d['max_div']:.3e} bound {bound:.3e}")
    assert d["max_div"] <= bound
    # the same pair with V's sign flipped is not divergence free: D = -(U s_x - V s_y) / N = -2 s_x s_y / N
    d2 = D.diagnostics(u, -v, w, np.ones_like(u), DT)
    assert d2["max_div"] > 100 * bound or N < 17


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_rigid_rotation_cfl(N, dtype):
    """u = -(j - c) s, v = (i - c) s, w = 0: cfl_x = |dt0 * u| at the row farthest from c, the product formed in T."""
    c, s = (N + 1) / 2.0, 0.125
    idx = np.arange(N + 2, dtype=np.float64)
    u = np.broadcast_to((-(idx - c) * s)[None, :, None], (N + 2,) * 3).astype(dtype)
    v = np.broadcast_to(((idx - c) * s)[None, None, :], (N + 2,) * 3).astype(dtype)
    w = np.zeros_like(u)
    d = D.diagnostics(u, v, w, np.ones_like(u), DT)
    dt0 = dtype(DT) * dtype(N)
    want = float(abs(dt0 * dtype((N - c) * s)))
    assert D.bits(d["cfl_x"]) == D.bits(want) and D.bits(d["cfl_y"]) == D.bits(want)
    assert D.bits(d["cfl_z"]) == D.bits(0.0) and D.bits(d["cfl"]) == D.bits(want)
    assert D.bits(d["max_speed"]) == D.bits(math.sqrt(2.0 * float(dtype((N - c) * s)) ** 2))
    # interior differences cancel exactly: u does not vary along i, v not along j
    assert D.bits(d["max_div"]) == D.bits(0.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_uniform_velocity_kinetic_energy(N, dtype):
    U, V, W = 0.5, -0.25, 0.125
    f = [np.full((N + 2,) * 3, val, dtype) for val in (U, V, W, 2.0)]
    d = D.diagnostics(*f, DT)
    want = 0.5 * (U * U + V * V + W * W)
    assert abs(d["kinetic"] - want) <= 2.0 ** -52 * want
    assert d["mass"] == 2.0 * N ** 3 and d["dens_min"] == 2.0 and d["dens_max"] == 2.0
    assert D.bits(d["max_speed"]) == D.bits(math.sqrt(U * U + V * V + W * W)) and d["nonfinite"] == 0
    # a general uniform velocity: every addition of the tree rounds once (SPEC §10), the squares are those of the
    # values as stored
    g = [np.full((N + 2,) * 3, val, dtype) for val in (0.3, -0.7, 0.11, 1.0)]
    a, b, c = (float(dtype(val)) for val in (0.3, -0.7, 0.11))
    want = 0.5 * (a * a + b * b + c * c)
    got = D.diagnostics(*g, DT)["kinetic"]
    assert abs(got - want) <= (D.sum_path_additions(N, dtype) + 4) * 2.0 ** -53 * want
