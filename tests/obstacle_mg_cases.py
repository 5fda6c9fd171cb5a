"""The mask families and cases that the tests of docs/SPEC.md §16 (obstacle-aware multigrid) share:
test_obstacles_mg_ref.py on the CPU and test_obstacles_mg_gpu.py on the device draw the same masks and right-hand sides,
so a case named on one side is the case of the other. Masks are (N+2)^3 arrays [k, j, i] of the dtype with noise on the
shell entries (§15: ignored). Importing this module needs no GPU and no libsfgpu.so."""
import numpy as np

import obstacle_cases as OC
import shape_cases as C

# box, random30, special, walls: the masks of obstacle_cases; the rest are about what coarsening does to a mask
FAMILIES = ("empty", "box", "random30", "special", "walls", "odd_box", "plate", "blocks", "seven_of_eight")
MIXED = ("odd_box", "seven_of_eight")  # families whose level 1 must hold cells with both kinds of children
TOL = 1e-3
DEFAULT = (2, 0, 8)   # (nu, max_levels, nu_c)
SHORT = (1, 2, 1)     # the first sweep, one restriction, one coarse sweep, one correction, one post-sweep
ITERS = 8             # max_iters of the solve cases
CHECK_EVERY = 4
# sf_precondition_masked: (N, dtype, setting, families). Levels 8, 4; 12, 6; 13: L = 1; 16: three levels; 34, 17;
# 40 ends at an odd 5; 64: five levels; 128 fp64 / 256 fp32: lane 63 holds the last cell of the row; 132 fp64 /
# 264 fp32: a second trip of the lane loop.
PRECONDITION = [
    (8, np.float32, DEFAULT, ("odd_box", "special")), (8, np.float64, DEFAULT, ("seven_of_eight",)),
    (12, np.float32, DEFAULT, ("blocks",)), (12, np.float64, DEFAULT, ("odd_box", "random30")),
    (13, np.float32, DEFAULT, ("box",)), (13, np.float64, DEFAULT, ("random30",)),
    (16, np.float32, DEFAULT, ("seven_of_eight", "plate")), (16, np.float64, DEFAULT, ("odd_box", "blocks")),
    (34, np.float32, DEFAULT, ("walls", "odd_box")), (34, np.float64, DEFAULT, ("random30",)),
    (40, np.float32, DEFAULT, ("odd_box",)), (40, np.float64, DEFAULT, ("seven_of_eight", "plate")),
    (64, np.float32, DEFAULT, ("odd_box", "empty")), (64, np.float64, DEFAULT, ("blocks", "walls")),
    (128, np.float64, DEFAULT, ("odd_box",)), (256, np.float32, DEFAULT, ("walls",)),
    (132, np.float64, SHORT, ("walls",)), (264, np.float32, SHORT, ("odd_box",)),
]
SOLVE_SIZES = (16, 34, 40, 64)
SOLVES = [(16, np.float32, "seven_of_eight"), (16, np.float64, "box"), (34, np.float32, "odd_box"),
          (34, np.float64, "walls"), (40, np.float32, "random30"), (40, np.float64, "odd_box"),
          (64, np.float32, "odd_box"), (64, np.float64, "plate")]
# (N, P, max_levels): every coarse level splits into whole planes per slab; each over both transports
# (34 over 2 admits one level only: nu_c masked sweeps on the fine grid, across a slab boundary)
DECOMPOSED = [(64, 4, 0), (64, 2, 0), (40, 2, 3), (34, 17, 0), (34, 2, 1)]
DECOMPOSED_ITERS = 4
DECOMPOSED_FAMILIES = ("blocks", "odd_box")  # blocks: solid coarse cells on both sides of the coarse slab boundaries
# a second sf_set_obstacles: (N, dtype, the first mask's family, the second's)
SECOND_MASK = (16, np.float32, "blocks", "odd_box")
# the measurements of §16.1: fp32, cg_velocity seed 500, DEFAULT against jacobi:8
COUNT_SEED, COUNT_LIMIT = 500, 400
STEP_K = 6


def seed(family, N):
    return 2500 + 17 * FAMILIES.index(family) + N


def case_id(N, dtype, family, s=DEFAULT):
    return f"{family}-N{N}-{C.dname(dtype)}-nu%d-L%d-c%d" % s


def mask(family, N, dtype, P=None):
    if family in OC.FAMILIES:
        return OC.mask(family, N, dtype, P)
    rng = np.random.RandomState(seed(family, N))
    m = np.zeros((N + 2,) * 3, dtype)
    In = m[1:-1, 1:-1, 1:-1]
    n2 = N // 2
    if family == "odd_box":
        # two overlapping boxes whose faces sit at odd positions (first cell even, last cell odd, 1-based): every face
        # cuts the pairs (2I-1, 2I), and the concave edges and corners of the union leave 1 to 7 solid children
        a = 2 * max(1, N // 8)
        b = a + 2 * max(1, N // 6) + 1
        s = 2 * max(1, N // 16)  # (even: the second box is misaligned like the first)
        m[a:b + 1, a:b + 1, a:b + 1] = 1
        m[a + s:b + s + 1, a + s:b + s + 1, a + s:b + s + 1] = 1
        m[a + s:b + 1, a:a + s, a + s:b + 1] = 0  # a notch through one face of the first box: concave corners
    elif family == "plate":
        # one cell thick across the whole box at plane k = N / 2, with a 4 x 4 hole (2 x 2 below N = 16): no coarse
        # cell keeps eight solid children, so the plate is gone from level 1 on
        k, h = N // 2, (4 if N >= 16 else 2)
        m[k, 1:-1, 1:-1] = 1
        m[k, n2 - h // 2 + 1:n2 + h // 2 + 1, n2 - h // 2 + 1:n2 + h // 2 + 1] = 0
    elif family in ("blocks", "seven_of_eight"):
        # 2 x 2 x 2 blocks on a fifth of the coarse cells: the coarse mask is exact; seven_of_eight frees one child each
        chosen = rng.random_sample((n2,) * 3) < 0.2
        chosen[n2 // 2, n2 // 2, n2 // 2] = True
        In[:2 * n2, :2 * n2, :2 * n2] = np.repeat(np.repeat(np.repeat(chosen, 2, 0), 2, 1), 2, 2)
        if family == "seven_of_eight":
            for K, J, Ic in np.argwhere(chosen):
                dk, dj, di = rng.randint(0, 2, 3)
                In[2 * K + dk, 2 * J + dj, 2 * Ic + di] = 0
    else:
        raise KeyError(family)
    return OC._shell_noise(m, rng)


def rhs_fields(family, N, dtype):
    """(z0, r) of a sf_precondition_masked case: standard normal on all (N+2)^3 entries, no set_bnd, so whatever z held
    and the shells of r are numbers a correct z never shows; r is not zero in solid cells."""
    rng = np.random.RandomState(seed(family, N) + 9000)
    return tuple(rng.standard_normal((N + 2,) * 3).astype(dtype) for _ in range(2))


def velocity(family, N, dtype):
    return C.cg_velocity(N, dtype, seed(family, N) + 5000)


def children_histogram(solid):
    """How many coarse cells of the next level have 0, 1, ..., 8 solid children (solid: interior-shaped, even n)."""
    lo, hi = slice(0, None, 2), slice(1, None, 2)
    count = sum(solid[k, j, i].astype(np.int64) for k in (lo, hi) for j in (lo, hi) for i in (lo, hi))
    return np.bincount(count.ravel(), minlength=9)


def count_mask(kind, N, dtype=np.float32):
    """The masks of the iteration counts of §16.1: empty; box, the cells N/3+1 .. 2N/3 per axis; sphere, the cells whose
    centre index lies within N/5 of the centre ((N+1)/2 per axis); plate, one cell thick at k = N/2 with a 4 x 4 hole."""
    m = np.zeros((N + 2,) * 3, dtype)
    if kind == "box":
        m[N // 3 + 1:2 * N // 3 + 1, N // 3 + 1:2 * N // 3 + 1, N // 3 + 1:2 * N // 3 + 1] = 1
    elif kind == "sphere":
        x = np.arange(N + 2) - (N + 1) / 2.0
        m[...] = (x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) <= (N / 5.0) ** 2
    elif kind == "plate":
        m[N // 2, :, :] = 1
        m[N // 2, N // 2 - 1:N // 2 + 3, N // 2 - 1:N // 2 + 3] = 0
    elif kind != "empty":
        raise KeyError(kind)
    return m
