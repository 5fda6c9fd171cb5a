"""The mask families and sizes that the tests of docs/SPEC.md §15 (solid obstacles) share: test_obstacles_ref.py on
the CPU and test_obstacles_gpu.py on the device draw the same masks, so a case named on one side is the case of the
other. Masks are (N+2)^3 arrays [k, j, i] of the dtype; what they hold on shell entries is noise on purpose (§15: shell
entries are ignored)."""
import numpy as np

import shape_cases as C

FAMILIES = ("empty", "box", "random30", "walls", "all_solid", "one_fluid", "special")
DEGENERATE = ("all_solid", "one_fluid")  # families whose fluid share is below a quarter by construction
SIZES = [1, 2, 3, 5, 13, 34, 65, 70]
SHAPES = [(N, t) for N in SIZES for t in C.DTYPES]
# single applications: the sizes above and the ones whose rows take a second trip of the lane loop
RESIDUAL_SHAPES = SHAPES + [(N, np.float64) for N in (130, 131)] + [(N, np.float32) for N in (257, 260, 262)]
ITERS = 8            # max_iters of the projection cases
CHECK_EVERY = 4      # the device-scalar form of those cases
SWEEPS = 2           # jacobi:2
TOL = 1e-3
CONVERGENCE_N = 34
STEP_N, STEP_K = 40, 6


def seed(family, N):
    return 1500 + 17 * FAMILIES.index(family) + N


def box_range(N):
    """The centred box: the cells i with 0.3 N < i <= 0.6 N per axis, as (first, last), 1-based (N = 1: none)."""
    return int(0.3 * N) + 1, int(0.6 * N)


def _shell_noise(mask, rng):
    """Positive values on every shell entry: a shell entry taken for a solid cell changes the result."""
    noise = (1.0 + rng.random_sample(mask.shape)).astype(mask.dtype)
    inner = np.zeros(mask.shape, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    return np.where(inner, mask, noise)


def seam_planes(N, dtype, slabs=(2, 4, 5, 17)):
    """Indices (1-based) on both sides of each 64-lane seam of a row (lane 63 | lane 0 of the next trip is the only
    seam inside a row: every 64 W cells) and of every slab boundary for the slab counts in use."""
    W = 16 // np.dtype(dtype).itemsize
    at = set()
    for s in range(64 * W, N, 64 * W):
        at.update((s, s + 1))
    for P in slabs:
        if N % P == 0:
            for b in range(N // P, N, N // P):
                at.update((b, b + 1))
    return sorted(x for x in at if 1 <= x <= N)


def mask(family, N, dtype, P=None):
    """The mask of a family at size N. P: the slab count whose boundaries `walls` must straddle (besides the defaults)."""
    rng = np.random.RandomState(seed(family, N))
    m = np.zeros((N + 2,) * 3, dtype)
    In = m[1:-1, 1:-1, 1:-1]
    if family == "empty":
        pass
    elif family == "box":
        lo, hi = box_range(N)
        m[lo:hi + 1, lo:hi + 1, lo:hi + 1] = 1
    elif family == "random30":
        In[...] = rng.random_sample(In.shape) < 0.3
    elif family == "walls":
        # a sparse coat of solid cells on every face, edge and corner of the interior, and on the planes either side of
        # each lane seam and slab boundary
        coat = np.zeros(In.shape, bool)
        for a in range(3):
            for side in (0, -1):
                idx = [slice(None)] * 3
                idx[a] = side
                coat[tuple(idx)] = True
        slabs = (2, 4, 5, 17) + ((P,) if P else ())
        for x in seam_planes(N, dtype, slabs):
            coat[x - 1, :, :] = True   # planes next to a slab boundary
            coat[:, :, x - 1] = True   # cells next to a lane seam
        In[...] = coat & (rng.random_sample(In.shape) < 0.5)
        corners = [(a, b, c) for a in (0, -1) for b in (0, -1) for c in (0, -1)]
        if N >= 5:
            for c in corners[::2]:
                In[c] = 1
        else:
            In[-1, -1, -1] = 0  # (the smallest grids are all wall: one cell stays fluid for certain)
    elif family == "all_solid":
        In[...] = 1
    elif family == "one_fluid":
        In[...] = 1
        In[tuple(rng.randint(0, N, 3))] = 0
    elif family == "special":
        tiny = np.finfo(dtype).smallest_subnormal
        values = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, -1.5, tiny, -tiny, 2.0], dtype)
        In[...] = values[rng.randint(0, len(values), In.shape)]
        In[0, 0, 0] = np.nan  # (fluid: the one cell of N = 1 too)
    else:
        raise KeyError(family)
    return _shell_noise(m, rng)


def parked_nan(fields, mk_solid):
    """Copies of the fields with a NaN in every solid interior cell."""
    out = []
    for x in fields:
        x = x.copy()
        x[1:-1, 1:-1, 1:-1][mk_solid] = np.nan
        out.append(x)
    return out
