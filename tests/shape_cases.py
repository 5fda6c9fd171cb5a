"""The case table and the input builders shared by tests/test_shape_inputs_ref.py (CPU: the inputs discriminate) and
tests/test_operator_shapes_gpu.py (GPU: forces, MacCormack, reductions at every shape and kernel form), and their
counterparts for the conjugate-gradient projection of SPEC §11: tests/test_pressure_cg_inputs_ref.py (CPU) and
tests/test_pressure_cg_shapes_gpu.py (GPU).

Sizes: 1, 2, 3 (every interior cell is an edge and a corner), 5, 13, 31, 34 (less than a wave, ragged vectors), 64 (one
full wave), 65 (one cell of a second wave; the plane fold pads to 128), 70, 130, 200 (two to four waves with a ragged
last one). 260 and 324 (fp32) and 130, 200 (fp64) take the second trip of the SPEC §10 row partial (N > 64 W).

CG_SHAPES adds the sizes around the end of a row's first stretch of 64 W cells, where the §11 stencil changes the cell
it takes as a lane's neighbour: N = 64 W exactly (128 fp64, 256 fp32: lane 63 takes the shell cell, no second trip),
64 W + 1 (129, 257: the second trip is one ragged vector that holds the shell cell itself), a full vector plus a ragged
one in the second trip (131, 262) and a second trip of many lanes (200 fp64, 324 fp32). With the shared sizes every
residue of N mod W occurs in both precisions."""
import numpy as np

DT = 0.1
DTYPES = [np.float32, np.float64]
SIZES = [1, 2, 3, 5, 13, 31, 34, 64, 65, 70, 130, 200]
REDUCE_ONLY_F32 = [260, 324]
SHAPES = [(N, dt) for N in SIZES for dt in DTYPES]
REDUCE_SHAPES = SHAPES + [(N, np.float32) for N in REDUCE_ONLY_F32]
CG_SHAPES = (SHAPES + [(N, np.float64) for N in (128, 129, 131)] + [(N, np.float32) for N in (256, 257, 262, 324)])
DECOMPOSED = [(34, 2, "copy"), (34, 17, "rccl-self"), (65, 5, "copy"), (70, 2, "rccl-self"), (130, 2, "copy"),
              (130, 5, "rccl-self"), (200, 4, "copy")]


def second_trip(N, dtype):
    """The SPEC §10 row partial takes m >= 1 (a lane adds more than one vector)."""
    return N > 64 * (16 // np.dtype(dtype).itemsize)


def cg_iters(N):
    """max_iters of the random-velocity solves: the numpy reference of a case stays at seconds (15 s for 324 fp32 at 3
    iterations, 5 s for 200 fp64 at 4)."""
    return 8 if N <= 130 else 4 if N <= 200 else 3


# Seeds of the random-velocity solves: 500 + N, except where another seed makes the solve tell a mean divided in fp32,
# (T)s / (T)N^3, from the mu of SPEC §11, (T)(s / N^3) (tests/test_pressure_cg_inputs_ref.py: one ulp of mu reaches r only
# where it flips the rounding of div - mu in some cell).
CG_SEEDS = {5: 508, 13: 532, 31: 535, 34: 500, 65: 584, 70: 503}


def cg_seed(N):
    return CG_SEEDS.get(N, 500 + N)


# Seeds of stored_shell_pair. poisson_residual is the square root of a ratio of two sums, and a last-bit change of a sum
# often does not reach it: at these sizes 900 + N does not show a second trip added in the wrong order, these seeds do.
CG_SHELL_SEEDS = {131: 1034, 200: 1103, 262: 1163, 324: 1225}


def shell_seed(N):
    return CG_SHELL_SEEDS.get(N, 900 + N)


def dname(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def smooth_flow(N):
    """The velocity of test_parity_gpu.test_advect_smooth_flow: traces of up to 2.5 cells that vary slowly along a
    row."""
    k, j, i = np.meshgrid(*(np.arange(N + 2, dtype=np.float64),) * 3, indexing="ij")
    amp = 2.5 / (DT * N)
    u = amp * np.sin(2 * np.pi * i / N + 0.3) * np.cos(2 * np.pi * j / N)
    v = amp * np.cos(2 * np.pi * (i + k) / N)
    w = amp * np.sin(2 * np.pi * (j - i) / N + 1.1)
    return u, v, w


def mixed_flow(N, dtype, seed):
    """(u, v, w): smooth_flow with, on one cell in sixteen, a normal perturbation of one cell (1 / (dt N) in velocity
    units). Along a row most neighbouring cells land in neighbouring cells and a share does not; traces reach the walls
    from a few cells away, and the roughness makes the limiter bite."""
    rng = np.random.RandomState(seed)
    out = []
    for c in smooth_flow(N):
        hit = rng.random_sample(c.shape) < 1.0 / 16.0
        out.append((c + hit * rng.standard_normal(c.shape) / (DT * N)).astype(dtype))
    return tuple(out)


def mixed_flow_one_plane(N, dtype, seed):
    """mixed_flow for decomposed contexts: w scaled so that |dt0 w| < 1 (one ghost plane, SPEC §4); u, v unchanged."""
    u, v, w = mixed_flow(N, dtype, seed)
    T = np.dtype(dtype).type
    w = (w.astype(np.float64) * (0.95 / float(np.abs(T(DT) * T(N) * w).max()))).astype(dtype)
    assert float(np.abs(T(DT) * T(N) * w).max()) < 1
    return u, v, w


def normal_field(N, dtype, seed, scale=1.0):
    return (scale * np.random.RandomState(seed).standard_normal((N + 2,) * 3)).astype(dtype)


def stored_shell_pair(N, dtype, seed):
    """(p, div): standard normal on all (N+2)^3 entries and no set_bnd, so that every shell cell differs from the cell
    it would mirror: a stencil that reads a neighbour "as stored" (SPEC §11) from the wrong cell reads another value."""
    rng = np.random.RandomState(seed)
    return tuple(rng.standard_normal((N + 2,) * 3).astype(dtype) for _ in range(2))


def cg_velocity(N, dtype, seed):
    """(u, v, w) for project_cg: 0.05-normal on all entries, shells as drawn."""
    rng = np.random.RandomState(seed)
    return [(0.05 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for _ in range(3)]


def decades_field(N, dtype, seed):
    """Magnitudes spread over five decades (test_diagnostics_gpu.test_every_op_and_the_struct_match_the_reference)."""
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((N + 2,) * 3) * 10.0 ** rng.randint(-2, 3, (N + 2,) * 3)).astype(dtype)


SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 0.0)


def special_values(x, rng, nonfinite=True):
    """A copy of x with, planted in its interior: NaN, +inf, -inf, -0.0, +0.0 — each on the first and the last cell of a
    row, on cells 64 and 65 where they exist, and on three random cells, every one in a row of its own choosing — and
    runs of equal values (ties): runs of one repeated value, and a block of non-negative data in which four cells in ten
    are zeros of either sign (-0 == +0 is the tie whose winner the SPEC §9 select forms fix). With nonfinite = False the
    NaN and infinities are left out. The block is planted first and kept clear of NaN so that the cells around it stay
    comparable."""
    x = x.copy()
    T = x.dtype.type
    N = x.shape[0] - 2
    side = min(N, 12)
    o = [1 + rng.randint(0, N - side + 1) for _ in range(3)]
    blk = tuple(slice(a, a + side) for a in o)
    sub = np.abs(x[blk])
    zero = rng.random_sample(sub.shape) < 0.4
    sub[zero] = np.where(rng.random_sample(sub.shape) < 0.5, T(-0.0), T(0.0))[zero]
    x[blk] = sub
    inside = np.zeros(x.shape, bool)
    inside[tuple(slice(max(a - 3, 0), a + side + 3) for a in o)] = True
    columns = [1, N] + [c for c in (64, 65) if c < N]
    def place(i, finite):
        """A cell (k, j, i), i random if None; a non-finite value stays three cells clear of the block (N >= 20)."""
        while True:
            c = (1 + rng.randint(N), 1 + rng.randint(N), i if i is not None else 1 + rng.randint(N))
            if finite or N < 20 or not inside[c]:
                return c

    for val in SPECIALS if nonfinite else SPECIALS[3:]:
        for i in columns + [None] * 3:
            x[place(i, np.isfinite(val))] = T(val)
    for start in columns + [1 + rng.randint(N) for _ in range(3)]:  # runs of one repeated value
        k, j = 1 + rng.randint(N), 1 + rng.randint(N)
        a = max(1, min(start - 1, N - 3))
        if not np.isfinite(x[k, j, a:min(a + 4, N + 1)]).all():
            continue
        x[k, j, a:min(a + 4, N + 1)] = x[k, j, a]
    return x


def forces_fields(N, dtype, seed):
    """The 8 named fields for the SPEC §8 operators: standard-normal velocities, 0.2-normal everything else, and (N >= 8)
    a block of zero velocity, inside which |omega| is uniform, its gradient zero and len = 0: there `tiny` alone keeps
    1 / (len + tiny) finite."""
    rng = np.random.RandomState(seed)
    names = ("u", "v", "w", "u0", "v0", "w0", "dens", "dens0")
    f = {n: (0.2 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in names}
    for n in ("u", "v", "w"):
        f[n] = rng.standard_normal((N + 2,) * 3).astype(dtype)
        if N >= 8:
            f[n][2:9, 3:10, N - 7:N + 1] = 0  # up to the last cell of the rows it crosses
    return f


def zero_coefficient_inputs(N, dtype):
    """forces_fields for the eps = 0 / beta = 0 cases of SPEC §8: -0 sources on every other interior cell of a row, NaN
    in the velocity and in dens."""
    f = forces_fields(N, dtype, 70 + N)
    for n in ("u0", "v0", "w0"):
        f[n][1:-1, 1:-1, 1:-1:2] = -0.0
    f["v"][1, 1, 1] = f["u"][N, N, N] = f["dens"][1, N, 1] = np.nan
    return f


# ---- inputs of the SPEC §3 operators and tracers held to bits (tests/stable_cases.py) ------------------------------
def wall_sites(N, rng):
    """Interior cells (k, j, i) that special_values meets only by luck: one on each of the six faces of the interior
    (i, j or k = 1 or N), one edge cell, one corner cell and, where N allows, cells 64 and 65 of a row: the last lane of
    a wave and the first of the next."""
    r = lambda: 1 + rng.randint(N)
    sites = [(r(), r(), 1), (r(), r(), N), (r(), 1, r()), (r(), N, r()), (1, r(), r()), (N, r(), r()),
             (N, 1, r()), (N, N, 1)]
    if N >= 65:
        k, j = r(), r()
        sites += [(k, j, 64), (k, j, 65)]
    return sites


def wall_specials(x, rng, nonfinite=True):
    """A copy of x with the values of SPECIALS planted at wall_sites: -0 and +0 on a cell of every site (a draw of
    sites each), and with nonfinite NaN, +inf and -inf too. From N = 64 on each non-finite value takes a draw of sites
    of its own; below, the three take turns over one draw, so that a small grid holds eight non-finite cells and a
    compared field does not drown in NaN."""
    x = x.copy()
    T = x.dtype.type
    N = x.shape[0] - 2
    for val in SPECIALS[3:]:
        for c in wall_sites(N, rng):
            x[c] = T(val)
    if nonfinite and N >= 64:
        for val in SPECIALS[:3]:
            for c in wall_sites(N, rng):
                x[c] = T(val)
    elif nonfinite:
        for q, c in enumerate(wall_sites(N, rng)):
            x[c] = T(SPECIALS[q % 3])
    return x


def zero_region(f, K, rng):
    """Copies of the fields of the dict f with two boxes of zeros, the same boxes in every field: one from the low i, j
    and k walls (shell included) 2K + 3 cells inward, clipped to N, of +0 and -0 with random signs; one of the same
    depth against the high walls, clipped to N / 2 so that it leaves the first standing, uniformly -0. Cells more than K from a box's inner faces stay zero through K sweeps,
    so their sign is what the SPEC's expression gives for zero operands."""
    out = {}
    for n, x in f.items():
        x = x.copy()
        T = x.dtype.type
        N = x.shape[0] - 2
        side = min(N, 2 * K + 3)
        lo = (slice(0, side + 1),) * 3
        x[lo] = np.where(rng.random_sample(x[lo].shape) < 0.5, T(-0.0), T(0.0))
        if N >= 2:
            x[(slice(N + 1 - min(side, N // 2), N + 2),) * 3] = T(-0.0)
        out[n] = x
    return out


def subnormal_field(N, dtype, seed, huge=False, scale=1.0):
    """Normal data (of standard deviation `scale`) in which about one cell in eight is a subnormal of either sign (one in sixty-four the
    smallest one) and, with huge (set_bnd and add_source only: a sum of six of them overflows a sweep), one cell in
    sixty-four lies within a factor two of the largest finite value, so that an edge's A + B overflows."""
    rng = np.random.RandomState(seed)
    T = np.dtype(dtype).type
    fi = np.finfo(dtype)
    x = (scale * rng.standard_normal((N + 2,) * 3)).astype(dtype)
    sign = np.where(rng.random_sample(x.shape) < 0.5, T(-1), T(1))
    pick = rng.random_sample(x.shape)
    sub = (rng.random_sample(x.shape) * float(fi.tiny)).astype(dtype)  # below the smallest normal
    x = np.where(pick < 1.0 / 8.0, sign * sub, x)
    x = np.where(pick < 1.0 / 64.0, sign * T(fi.smallest_subnormal), x)
    if huge:
        big = (T(fi.max) * (0.5 + 0.5 * rng.random_sample(x.shape))).astype(dtype)
        x = np.where(pick > 1.0 - 1.0 / 64.0, sign * big, x)
    return x.astype(dtype)


LANDING_DT = 0.125


def exact_landing(N, dtype, seed, dt=LANDING_DT):
    """(d0, u, v, w) for advect with dt: velocities m / dt0 with m an integer in -3 .. 3 or, on one cell in eight, the
    half-integer that carries the cell onto lo = 0.5 or hi = N + 0.5. With dt = 0.125 and N a power of two dt0 is a
    power of two, every velocity exact, and the traces land exactly on cell centres (s1 = t1 = r1 = 0, also with
    i0 = N and clamped at lo) and on the two bounds. d0 is standard normal with a block of -0, and three cells (2, 2, c)
    whose trace is made to land on their own centre with d0 = -0 there and +inf, a negative and a positive value at the
    i0 + 1 sample, which the SPEC multiplies by s1 = 0: NaN, and +0 from -0 + (+0)."""
    rng = np.random.RandomState(seed)
    T = np.dtype(dtype).type
    dt0 = T(dt) * T(N)
    idx = np.arange(N + 2, dtype=np.float64)
    vel = []
    for ax in range(3):
        m = rng.randint(-3, 4, (N + 2,) * 3).astype(np.float64)
        shape = [1, 1, 1]
        shape[2 - ax] = N + 2
        pos = idx.reshape(shape)
        pick = rng.random_sample(m.shape)
        m = np.where(pick < 1.0 / 16.0, pos - 0.5, m)
        m = np.where(pick > 1.0 - 1.0 / 16.0, pos - (N + 0.5), m)
        vel.append(m)
    d0 = rng.standard_normal((N + 2,) * 3).astype(dtype)
    side = min(N, 4)
    d0[(slice(N + 1 - side, N + 1),) * 3] = T(-0.0)
    if N >= 8:
        for c, val in ((1, np.inf), (3, -1.5), (5, 2.5)):
            for m in vel:
                m[2, 2, c] = 0.0
            d0[2, 2, c] = T(-0.0)
            d0[2, 2, c + 1] = T(val)
    u, v, w = ((m / float(dt0)).astype(dtype) for m in vel)
    return d0, u, v, w


def tracer_positions(N, dtype, seed, n=200):
    """(n + specials, 3) positions: uniform over [-1, N + 2] and, cycled through the three coordinates of the rest,
    0.5, N + 0.5 and one ulp either side of each, integers, +-0, +-inf and NaN."""
    rng = np.random.RandomState(seed)
    T = np.dtype(dtype).type
    lo, hi = T(0.5), T(N) + T(0.5)
    edge = [lo, hi, np.nextafter(lo, T(0)), np.nextafter(lo, T(1)), np.nextafter(hi, T(0)), np.nextafter(hi, T(2 * N + 2)),
            T(0.0), T(-0.0), T(np.inf), T(-np.inf), T(np.nan), T(1), T(N), T(N + 1), T(max(N // 2, 1))]
    pos = rng.uniform(-1.0, N + 2.0, size=(n + 3 * len(edge), 3)).astype(dtype)
    for q, val in enumerate(edge):
        for ax in range(3):
            pos[n + 3 * q + ax, ax] = val
            pos[n + 3 * q + ax, (ax + 1) % 3] = edge[(q + ax + 1) % len(edge)] if q % 2 else pos[n + 3 * q + ax, (ax + 1) % 3]
    return pos
