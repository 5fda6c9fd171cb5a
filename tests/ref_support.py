"""What the CPU-side tests of the numpy references share: the product modes and the tolerance of the analytic pin
(docs/SPEC.md §7.1), the comparison and the mutated row partial of the input-discrimination tests, and the run of
BASELINE.json configs[0] that tests/golden/make_config1_golden.py records. No GPU and no libsfgpu.so needed."""
import numpy as np

import diagnostics_ref as D
import oracle_lib as O
from gpu_support import DIFF, DT, VISC

LD = np.longdouble


# ---- closed forms (tests/test_oracle_analytic.py explains them) -------------------------------------------------
def modes(N, m):
    i = np.arange(N + 2, dtype=LD)
    th = LD(np.pi) * LD(m) * (i - LD(0.5)) / LD(N)
    return np.cos(th), np.sin(th)


def product(fk, fj, fi):
    return fk[:, None, None] * fj[None, :, None] * fi[None, None, :]


def tol(dtype, K, scale):
    return 16.0 * (K + 2) * float(np.finfo(dtype).eps) * float(scale)


# ---- the inputs discriminate -------------------------------------------------------------------------------------
def same_bits(a, b):
    """Same positions NaN, every other entry the same bits (gpu_support.assert_same_bits with nan_ok, as a predicate)."""
    uint = np.uint32 if a.dtype == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(uint)[~na], b.view(uint)[~nb]))


def row_partials_one_trip(terms, W, drop=False):
    """Mutation 6 of tests/test_shape_inputs_ref.py: the lane stride of the first trip only; cells beyond 64 W are added
    to lane 0 one after another (drop: not added at all — the loop over m runs once)."""
    nk, N, _ = terms.shape
    first = min(N, D.LANES * W)
    t = np.zeros((nk, N, D.LANES * W), np.float64)
    t[:, :, :first] = terms[:, :, :first]
    t = t.reshape(nk, N, D.LANES, W)
    c = np.zeros((nk, N, D.LANES), np.float64)
    for e in range(W):
        c = c + t[:, :, :, e]
    for i in range(first, N if not drop else first):
        c[:, :, 0] = c[:, :, 0] + terms[:, :, i]
    return D.halve(c)


# ---- BASELINE.json configs[0] ------------------------------------------------------------------------------------
CONFIG1_N, CONFIG1_K = 32, 10


def run_config1():
    """One vel_step + dens_step of the CPU oracle at 32^3, K = 10, one density and one velocity source: (fields, density
    and velocity of the interior as the frame holds them)."""
    N = CONFIG1_N
    z = lambda: np.zeros((N + 2,) * 3, np.float32)
    f = {n: z() for n in ("u", "v", "w", "u0", "v0", "w0", "dens", "dens0")}
    c = N // 2
    f["dens0"][c, c, c] = 100.0
    f["v0"][c, c, c] = 5.0
    O.step(N, f, np.float32(DT), np.float32(DIFF), np.float32(VISC), CONFIG1_K)
    dens = np.ascontiguousarray(f["dens"][1:-1, 1:-1, 1:-1]).ravel()
    vel = np.stack([f["u"][1:-1, 1:-1, 1:-1], f["v"][1:-1, 1:-1, 1:-1], f["w"][1:-1, 1:-1, 1:-1]], -1).ravel()
    return f, dens, vel


def frame_args(path, ub, dens, vel):
    return (path, ub, [CONFIG1_N + 1] * 3, 2, [1, 3], [0, 0], ["density", "velocity"], [dens, vel])
