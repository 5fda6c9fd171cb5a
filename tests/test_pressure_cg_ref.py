"""The numpy reference of the conjugate-gradient projection (tests/pressure_cg_ref.py, docs/SPEC.md §11) pinned by closed
forms and by the measurement that motivates the operator. No GPU needed; tests/test_pressure_cg_gpu.py then holds
libsfgpu.so to this reference bit for bit."""
import numpy as np
import pytest

import diagnostics_ref as D
import pressure_cg_ref as R
from gpu_support import DTYPE_IDS, DTYPES
from ref_support import LD, modes, product, tol


def same(a, b):
    uint = np.uint32 if a.dtype == np.float32 else np.uint64
    return np.array_equal(a.view(uint), b.view(uint))


def mode_pair(N, m, amps, dtype):
    """u = U psi phi phi, v = V phi psi phi, w = W phi phi psi of §7.1 and the mode M = phi phi phi."""
    (cx, sx), (cy, sy), (cz, sz) = (modes(N, q) for q in m)
    U, V, W = amps
    f = (LD(U) * product(cz, cy, sx), LD(V) * product(cz, sy, cx), LD(W) * product(sz, cy, cx))
    return [np.ascontiguousarray(a.astype(dtype)) for a in f], product(cz, cy, cx), (product(cz, cy, sx), product(cz, sy, cx),
                                                                                    product(sz, cy, cx))


def few_shell(N):
    idx = np.arange(N + 2)
    shell = ((idx == 0) | (idx == N + 1)).astype(int)
    return (shell[:, None, None] + shell[None, :, None] + shell[None, None, :]) <= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N,m", [(8, (1, 1, 1)), (16, (2, 5, 3)), (12, (4, 0, 7))])
def test_a_single_mode_is_solved_in_one_iteration(N, m, dtype):
    """div = D M is an eigenvector of A with eigenvalue 6 - lambda: the first search direction is the answer."""
    amps = (0.6, -0.4, 0.9)
    (u, v, w), M, vel_modes = mode_pair(N, m, amps, dtype)
    out = R.project_cg(u, v, w, 1e-3, 50)
    assert (out["status"], out["iterations"]) == (R.CONVERGED, 1), (out["status"], out["iterations"], out["rel_residual"])
    pi = LD(np.pi)
    s = [np.sin(pi * q / N) for q in m]
    lam = 2 * sum(np.cos(pi * q / N) for q in m)
    Dm = -LD(dtype(0.5)) * LD(dtype(1) / dtype(N)) * 2 * sum(a * b for a, b in zip(amps, s))
    Pm = Dm / (6 - lam)
    assert float(np.max(np.abs(out["div"].astype(LD) - Dm * M))) <= tol(dtype, 2, 4.0 / N)
    assert float(np.max(np.abs(out["p"].astype(LD) - Pm * M))) <= tol(dtype, 1, 2 * abs(float(Dm)) / float(6 - lam) + 1e-30)
    few = few_shell(N)
    for name, a, sq, f in zip("uvw", amps, s, vel_modes):
        err = float(np.max(np.abs(out[name].astype(LD) - (a + N * Pm * sq) * f)[few]))
        assert err <= tol(dtype, 1, 2.0 + N * abs(float(Pm))), (name, err)
    assert R.poisson_residual(out["p"], out["div"]) <= 64 * float(np.finfo(dtype).eps)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_two_modes_take_two_iterations(dtype):
    N = 16
    (u1, v1, w1), _, _ = mode_pair(N, (2, 5, 3), (0.6, -0.4, 0.9), np.float64)
    (u2, v2, w2), _, _ = mode_pair(N, (1, 0, 2), (-0.3, 0.0, 0.5), np.float64)
    u, v, w = ((a + b).astype(dtype) for a, b in ((u1, u2), (v1, v2), (w1, w2)))
    out = R.project_cg(u, v, w, 1e-3, 50)
    assert (out["status"], out["iterations"]) == (R.CONVERGED, 2), (out["iterations"], out["rel_residual"])
    assert R.project_cg(u, v, w, 1e-3, 1)["status"] == R.MAX_ITERS


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_zero_velocity_is_left_alone(dtype):
    N = 9
    z = np.zeros((N + 2,) * 3, dtype)
    z[3, 4, 5] = -0.0  # a signed zero survives: u - c_grad*(0 - 0) = -0 - 0 = -0
    out = R.project_cg(z, z, z, 1e-3, 10)
    assert (out["status"], out["iterations"], out["rel_residual"]) == (R.CONVERGED, 0, 0.0)
    assert not out["p"].any() and not np.signbit(out["p"]).any()
    for n in "uvw":
        assert same(out[n][1:-1, 1:-1, 1:-1], z[1:-1, 1:-1, 1:-1])
    assert R.poisson_residual(out["p"], out["div"]) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_no_iterations_allowed(dtype):
    u, v, w = R.smooth_velocity(12, dtype)
    out = R.project_cg(u, v, w, 1e-3, 0)
    assert (out["status"], out["iterations"], out["rel_residual"]) == (R.MAX_ITERS, 0, 1.0)
    assert not out["p"].any()
    for n, f in zip("uvw", (u, v, w)):
        assert np.array_equal(out[n], f)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_nan_in_the_velocity_is_a_breakdown(dtype):
    u, v, w = R.smooth_velocity(12, dtype)
    u[5, 6, 7] = np.nan
    out = R.project_cg(u, v, w, 1e-3, 20)
    assert out["status"] == R.BREAKDOWN and out["iterations"] in (0, 1)
    assert np.isnan(out["rel_residual"])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", [8, 20])
def test_emulated_slabs_give_the_same_bits(N, dtype):
    rng = np.random.RandomState(N)
    u, v, w = ((0.05 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for _ in range(3))
    for b, f in ((1, u), (2, v), (3, w)):
        R.set_bnd(b, f)
    one = R.project_cg(u, v, w, 1e-2, 6)
    for slabs in (2, 4):
        out = R.project_cg(u, v, w, 1e-2, 6, slabs=slabs)
        assert all(same(out[n], one[n]) for n in ("u", "v", "w", "p", "div"))
        assert (out["status"], out["iterations"]) == (one["status"], one["iterations"])
        assert D.bits(out["rel_residual"]) == D.bits(one["rel_residual"])
        assert D.bits(R.poisson_residual(out["p"], out["div"], slabs)) == D.bits(R.poisson_residual(one["p"], one["div"]))


def test_set_bnd_is_the_oracles():
    import oracle_lib as O

    rng = np.random.RandomState(3)
    for N in (1, 2, 7):
        for b in range(4):
            x = rng.standard_normal((N + 2,) * 3).astype(np.float32)
            y = x.copy()
            O.set_bnd(b, y)
            assert same(R.set_bnd(b, x), y)


def test_jacobi_reference_is_the_oracles_project():
    import oracle_lib as O

    u, v, w = R.smooth_velocity(10, np.float32)
    want = [f.copy() for f in (u, v, w)] + [np.zeros_like(u), np.zeros_like(u)]
    O.project(*want, 7)
    out = R.project_jacobi(u, v, w, 7)
    for n, f in zip(("u", "v", "w", "p", "div"), want):
        assert same(out[n], f), n


# measured with this reference (the real §10 tree): N, iterations, recurrence residual, poisson_residual after CG at
# tol = 1e-3, poisson_residual after Jacobi K = 20
MEASURED = {
    (32, "f32"): (11, 6.0999638664e-04, 6.1001034990e-04, 0.7740831957),
    (64, "f32"): (22, 9.7391605001e-04, 9.7804535852e-04, 0.9362500150),
    (32, "f64"): (3, 3.2419386432e-09, 3.2419379151e-09, 0.7740831405),
}


@pytest.mark.parametrize("N,dtype", [(32, np.float32), (64, np.float32), (32, np.float64)], ids=["32-f32", "64-f32", "32-f64"])
def test_cg_solves_what_twenty_jacobi_sweeps_do_not(N, dtype):
    """The motivation of §11 on the smooth field, re-measured with the real sum tree. Values this reference gives:

        N   T    CG iterations  recurrence  poisson_residual (CG)  poisson_residual (Jacobi K = 20)
        32  f32  11             6.0999e-04  6.1001e-04             0.77408
        64  f32  22             9.7392e-04  9.7805e-04             0.93625
        32  f64   3             3.2419e-09  3.2419e-09             0.77408

    fp32 takes 11 and 22 iterations, as with plain sums. fp64 at N = 32 takes 3, not 11: the field is a sum of four
    eigenmodes of A, which exact arithmetic solves in four iterations (three reach 1e-3); in fp32 the rounding of the
    input spreads the right-hand side over every mode."""
    name = "f32" if dtype == np.float32 else "f64"
    tol_cg = 1e-3
    u, v, w = R.smooth_velocity(N, dtype)
    jac = R.project_jacobi(u, v, w, 20)
    res_j = R.poisson_residual(jac["p"], jac["div"])
    out = R.project_cg(u, v, w, tol_cg, 64)
    res_c = R.poisson_residual(out["p"], out["div"])
    div0 = D.reduce("max_abs", out["div"])
    div_j = D.reduce("max_abs", R.divergence(jac["u"], jac["v"], jac["w"])[1])
    div_c = D.reduce("max_abs", R.divergence(out["u"], out["v"], out["w"])[1])
    print(f"N={N} {name}: jacobi K=20 residual {res_j:.10g} max_div ratio {div_j / div0:.4g}; cg iterations "
          f"{out['iterations']} recurrence {out['rel_residual']:.10e} true {res_c:.10e} max_div ratio {div_c / div0:.4g}")
    assert res_j >= 0.5
    assert out["status"] == R.CONVERGED
    assert res_c <= 4 * tol_cg
    assert out["rel_residual"] <= tol_cg
    its, rec, true, jres = MEASURED[(N, name)]
    assert out["iterations"] == its
    assert abs(out["rel_residual"] - rec) <= 1e-6 * rec and abs(res_c - true) <= 1e-6 * true and abs(res_j - jres) <= 1e-6
    assert div_c <= 0.05 * div0 < div_j
