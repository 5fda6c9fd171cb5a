"""The inputs and the conditions that the tests of docs/SPEC.md §17 (mask-aware transport) share:
test_obstacle_transport_ref.py on the CPU and test_obstacle_transport_gpu.py on the device draw the same masks (those of
tests/obstacle_cases.py), fields and velocities, so a case named on one side is the case of the other."""
import numpy as np

import obstacle_cases as OC
import obstacles_ref as OB
import shape_cases as C
import stable_ref as S3

DT = C.DT
FAMILIES = ("empty", "box", "random30", "walls", "special", "all_solid", "one_fluid")
MIXED = ("box", "random30", "walls", "special")  # families with fluid cells next to solid ones
SIZES = OC.SIZES
BS = (0, 1, 2, 3)
SWEEPS = (1, 2, 5)
A = 0.1  # the Jacobi coefficient of the conservation cases
# the row shapes of the sweep (all random30): second trips of the lane loop and ragged last vectors
ROW_SHAPES = [(N, np.float64, 1) for N in (128, 129, 131, 200)] + [(N, np.float32, 2) for N in (256, 257, 262)]
# (N, P) of the decomposed cases
DECOMPOSED = [(34, 2), (34, 17), (64, 4), (40, 2)]
DIFF = 0.02  # a = dt diff N^2: 0.34 at N = 13, 2.3 at N = 34 (the solve matters)


def seed(family, N, b=0):
    return 7000 + 101 * FAMILIES.index(family) + 7 * N + b


def fields(family, N, dtype, b=0):
    """(x, x0): standard normal on all (N+2)^3 entries, no set_bnd: the stored shells are independent random numbers."""
    rng = np.random.RandomState(seed(family, N, b))
    return [rng.standard_normal((N + 2,) * 3).astype(dtype) for _ in range(2)]


def velocity(family, N, dtype, one_plane=False):
    """(u, v, w) on all entries: normal with dt0 * sigma = 0.6 plus a drift of 0.4 cells away from the centre of the grid
    on every axis, so that a share of the traces is longer than one cell, a share reaches the walls, and the traces of
    the cells round a centred obstacle land in it. one_plane (decomposed contexts, SPEC §4): w clipped to
    |dt0 w| <= 0.9."""
    rng = np.random.RandomState(seed(family, N) + 50000)
    dt0 = DT * N
    k, j, i = np.meshgrid(*(np.arange(N + 2) - (N + 1) / 2,) * 3, indexing="ij")
    u, v, w = [((0.6 * rng.standard_normal((N + 2,) * 3) + 0.4 * np.sign(g)) / dt0).astype(dtype) for g in (i, j, k)]
    if one_plane:
        w = np.clip(w, -0.9 / dt0, 0.9 / dt0).astype(dtype)
    return u, v, w


def far_velocity(family, N, dtype):
    """velocity() for two slabs with one cell, on the last plane of the first slab, whose trace crosses 6.5 planes into
    the second: more than the ghost planes a slab stores (four at most), so the halo condition of §4 is violated."""
    u, v, w = velocity(family, N, dtype, one_plane=True)
    w[N // 2, N // 2, N // 2] = -6.5 / (DT * N)
    return u, v, w


def advect_facts(mask, vel, slabs=1):
    """What test_conditions_hold looks at, on the mask and velocity of the compared case: (fluid cells that take at least
    one solid sample, the most traces longer than one cell on one of `slabs` k-slabs)."""
    N, dtype = mask.shape[0] - 2, mask.dtype
    mk = OB.Mask(mask)
    solid = OB.solid_cells(mask)
    T = np.dtype(dtype).type
    (i0, j0, k0), (x, y, z) = S3.SPEC.trace(vel, T(DT) * T(N))
    hit = np.zeros((N,) * 3, bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                hit |= solid[k0 + dk, j0 + dj, i0 + di]
    k, j, i = np.meshgrid(*(np.arange(1, N + 1, dtype=np.float64),) * 3, indexing="ij")
    with np.errstate(invalid="ignore"):
        far = (np.abs(x - i) > 1) | (np.abs(y - j) > 1) | (np.abs(z - k) > 1)
    nzl = N // slabs
    per_slab = [int(far[s * nzl:(s + 1) * nzl].sum()) for s in range(slabs)]
    return int((hit & mk.fluid).sum()), max(per_slab)
