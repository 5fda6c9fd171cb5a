"""The inputs and the conditions that the tests of docs/SPEC.md §19 (moving solids) share:
test_obstacle_moving_ref.py on the CPU and test_obstacle_moving_gpu.py on the device draw the same masks (those of
tests/obstacle_cases.py), fields and velocities (those of tests/obstacle_transport_cases.py) and solid velocities, so a
case named on one side is the case of the other."""
import numpy as np

import obstacle_cases as OC
import obstacle_moving_ref as MR
import obstacle_transport_cases as TC
import obstacles_ref as OB
import shape_cases as C
from gpu_support import DIFF as STEP_DIFF, VISC, random_fields

DT = C.DT
FAMILIES = ("box", "random30", "walls", "special", "all_solid", "one_fluid")
MIXED = TC.MIXED  # families with fluid cells next to solid ones
DEGENERATE = OC.DEGENERATE
SIZES = OC.SIZES
BS = TC.BS
SWEEPS = TC.SWEEPS
DIFF = TC.DIFF  # of the single diffusions; the steps run with gpu_support.DIFF (STEP_DIFF)
ITERS = OC.ITERS  # max_iters of the projection cases
TOL = OC.TOL
# (name, m, mg): plain CG, jacobi:2 and the masked V-cycle (nu, max_levels, nu_c)
SOLVERS = (("cg", 0, None), ("jacobi2", 2, None), ("mg", 0, (2, 0, 8)))
# the second trip of a row: (N, dtype)
ROW_SHAPES = [(129, np.float64), (131, np.float64), (257, np.float32), (262, np.float32)]
DECOMPOSED = TC.DECOMPOSED


def seed(family, N):
    return 19000 + 211 * OC.FAMILIES.index(family) + 5 * N


def project_fields(family, N, dtype):
    """(u, v, w): normal, sigma 0.2, on all (N+2)^3 entries, no set_bnd."""
    rng = np.random.RandomState(seed(family, N) + 1)
    return [(0.2 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for _ in range(3)]


def solid_velocity(family, N, dtype, scale=0.2):
    """(us, vs, ws): three independent normal fields of the velocity's scale, one value per cell and component on all
    (N+2)^3 entries, so that the wrong cell and the wrong component both show."""
    rng = np.random.RandomState(seed(family, N) + 2)
    return [(scale * rng.standard_normal((N + 2,) * 3)).astype(dtype) for _ in range(3)]


def transport_scale(N):
    """The sigma of obstacle_transport_cases.velocity: dt0 sigma = 0.6 cells."""
    return 0.6 / (DT * N)


def parked(vs, mask):
    """Copies of the solid velocity with a NaN in every fluid and shell entry: only interior solid cells keep a value."""
    solid = OB.solid_cells(mask)
    return [np.where(solid, x, x.dtype.type(np.nan)) for x in vs]


def zero_velocity(N, dtype):
    return [np.zeros((N + 2,) * 3, dtype) for _ in range(3)]


def row_mask(N, dtype):
    """random30 with solid cells planted so that, in every row, the cells 64 W and 64 W + 1 (both sides of the lane
    seam) and the last cell of the row are fluid cells with closed faces or solid cells, alternating by row."""
    m = OC.mask("random30", N, dtype)
    W = 16 // np.dtype(dtype).itemsize
    In = m[1:-1, 1:-1, 1:-1]
    s = 64 * W  # 1-based index of the last cell of the first trip
    rows = (np.arange(N)[:, None] + np.arange(N)[None, :]) % 4  # [k, j]
    for idx, pattern in ((s - 1, (1, 0, 1, 0)), (s, (0, 1, 1, 0)), (N - 1, (1, 0, 0, 1)), (N - 2, (0, 1, 0, 1))):
        In[:, :, idx] = np.asarray(pattern, dtype)[rows]
    return m


def row_fields(N, dtype, count, scale=0.2):
    """`count` normal fields for the row-shape cases, drawn in the dtype itself (their grids have up to 18 million
    entries)."""
    rng = np.random.default_rng(seed("random30", N) + 3)
    if np.dtype(dtype) == np.float32:
        return [np.float32(scale) * rng.standard_normal((N + 2,) * 3, dtype=np.float32) for _ in range(count)]
    return [scale * rng.standard_normal((N + 2,) * 3) for _ in range(count)]


def closed_face_cells(mask):
    """Fluid cells with a closed face on axis i, j, k."""
    mk = OB.Mask(mask)
    return tuple(int(((mk.closed[a + "lo"] | mk.closed[a + "hi"]) & mk.fluid).sum()) for a in "ijk")


def fluid_share(mask):
    mk = OB.Mask(mask)
    return mk.n_fluid / float(mk.fluid.size)


advect_facts = TC.advect_facts


def moved_box(N, dtype, shift):
    """The centred box of obstacle_cases moved `shift` cells along i."""
    lo, hi = OC.box_range(N)
    m = np.zeros((N + 2,) * 3, dtype)
    m[lo:hi + 1, lo:hi + 1, lo + shift:hi + 1 + shift] = 1
    return m


MOVED_N, MOVED_K = 13, 4


def moved_box_sequence(dtype=np.float32, N=MOVED_N, K=MOVED_K):
    """Two vel_step + dens_step pairs with the centred box of step 0 moved one cell along i for step 1, mask and solid
    velocity set again in between. Returns [(mask, vs, vel outcome, dens), ...]; the GPU file runs the same sequence."""
    f = random_fields(N, dtype, 190)
    speed = dtype(1.0 / (DT * N))  # one cell per step along i
    vs = [np.full((N + 2,) * 3, speed, dtype), np.zeros((N + 2,) * 3, dtype), np.zeros((N + 2,) * 3, dtype)]
    g, outs = dict(f), []
    for step in range(2):
        mask = moved_box(N, dtype, step)
        proj = lambda u, v, w: MR.project_cg(u, v, w, mask, vs, 1e-2, 10)  # noqa: E731
        vel = MR.vel_step(g, mask, vs, K, DT, VISC, proj)
        dens = MR.dens_step(g["dens"], f["dens0"], vel["u"], vel["v"], vel["w"], mask, K, DT, STEP_DIFF)
        outs.append((mask, vs, vel, dens))
        g = dict(f, u=vel["u"], v=vel["v"], w=vel["w"], dens=dens)
    return outs
