"""The cases of tests/test_stable_bits_gpu.py (GPU: the SPEC §3 operators and the tracers against the C++ oracle, bit
for bit, special values included) and of tests/test_stable_inputs_ref.py (CPU: the numpy statement of §3 equals the
oracle on these inputs, the inputs tell eight mutants from it, and no case drowns in NaN): the case tables, the inputs
built from tests/shape_cases.py, and the NaN-share condition. Needs no GPU and no libsfgpu.so.

The NaN-share condition: a comparison says little once NaN has spread over the field, so every compared field of
every case must have NaN on fewer than a quarter of its interior cells *in the reference*. A K-sweep ball holds
(2K+1)(2K^2+2K+3)/3 cells; hence non-finite values only from N = 13 on (one hand-placed N = 5 case apart), eight
non-finite cells and K <= 4 up to N = 34, and in the full steps two NaN, both in the density, which no velocity reads."""
import numpy as np

import shape_cases as C
from shape_cases import DT

A_LIN, C_LIN = 0.37, 1 + 6 * 0.37
FAMILIES = ("specials", "zeros", "subnormal")
SIZES_K = [N for N in C.SIZES if N <= 130]

# (N, K) of lin_solve: odd and even K in 1..7 (single, pair and four-sweep passes all end a solve somewhere)
LIN_CASES = [(1, 1), (2, 2), (3, 3), (5, 4), (5, 7), (13, 4), (13, 5), (31, 3), (31, 6), (34, 2), (34, 7), (64, 1),
             (64, 4), (64, 7), (65, 5), (65, 6), (70, 3), (70, 7), (130, 2), (130, 7)]
LIN_BIG = [(200, 4, np.float64), (260, 4, np.float32)]
LIN_SWITCH_CASES = [(34, 7), (64, 4), (65, 5), (130, 7)]
LIN_SWITCHES = [{"SF_MARCH": "0"}, {"SF_SK_S": "2"}, {"SF_SK_S": "3"}, {"SF_OVL": "0"}, {"SF_OVL": "2"}]
# (N, K) of project: K = 1, 2, 5, 8 and K = 0 (the two halves alone, on p = 0)
PROJECT_CASES = [(1, 1), (2, 2), (3, 5), (5, 8), (5, 0), (13, 2), (31, 5), (34, 8), (34, 0), (64, 8), (64, 1), (65, 5),
                 (70, 2), (130, 8)]
ADVECT_BIG = [(200, np.float64), (260, np.float32)]
LANDING_CASES = [(8, C.LANDING_DT), (64, C.LANDING_DT), (128, C.LANDING_DT), (65, DT), (70, DT)]
STEP_K = 3
STEP_CASES = [(N, P, bound, state) for N in (34, 64) for P in (1, 2) for bound in (False, True)
              for state in ("config1", "random")]
TRACER_SIZES = [4, 16, 33]


def nan_share(x):
    inner = x[(slice(1, -1),) * 3] if x.ndim == 3 else x
    return float(np.isnan(inner).mean())


def check_nan_share(fields, what):
    """The condition of the module docstring on the reference's fields (a dict or a list of arrays)."""
    items = fields.items() if isinstance(fields, dict) else enumerate(fields)
    for n, x in items:
        share = nan_share(x)
        assert share < 0.25, f"{what}: {n}: NaN on {share:.3f} of the reference's interior cells: the case is vacuous"


def nonfinite_at(N, K=0):
    return N >= 13 and (K <= 4 or N >= 64)


def specials(N, dtype, rng, seed, nonfinite, everywhere=True):
    """special_values + wall_specials of a normal field. Below N = 64 only wall_specials plants non-finite values."""
    x = C.special_values(C.normal_field(N, dtype, seed), rng, bool(nonfinite and everywhere and N >= 64))
    return C.wall_specials(x, rng, bool(nonfinite and (everywhere or N < 64)))


def pointwise_inputs(N, dtype, family):
    """(x, s) of add_source / set_bnd: the subnormal family with the huge values."""
    rng = np.random.RandomState(1000 + N)
    if family == "subnormal":
        return C.subnormal_field(N, dtype, N, huge=True), C.subnormal_field(N, dtype, N + 1, huge=True)
    if family == "zeros":
        z = C.zero_region({"x": C.normal_field(N, dtype, N), "s": C.normal_field(N, dtype, N + 1)}, 1, rng)
        return z["x"], z["s"]
    nf = nonfinite_at(N)
    return specials(N, dtype, rng, N, nf), specials(N, dtype, rng, N + 1, nf)


def lin_inputs(N, dtype, family, K, nonfinite=None):
    """(x, x0) of lin_solve. The subnormal family is scaled to the bottom of the normal range, so that the sums and
    products of a sweep land among the subnormals too."""
    rng = np.random.RandomState(2000 + N + K)
    if family == "subnormal":
        s = 4 * float(np.finfo(dtype).tiny)
        return C.subnormal_field(N, dtype, N, scale=s), C.subnormal_field(N, dtype, N + 1, scale=s)
    if family == "zeros":
        z = C.zero_region({"x": C.normal_field(N, dtype, N), "x0": C.normal_field(N, dtype, N + 1)}, K, rng)
        return z["x"], z["x0"]
    nf = nonfinite_at(N, K) if nonfinite is None else nonfinite
    return specials(N, dtype, rng, N, nf), specials(N, dtype, rng, N + 1, nf, everywhere=False)


def lin_n5_nonfinite(dtype):
    """The one N = 5 case with non-finite values: (x, x0, K) with a NaN in a corner cell of x0, +inf on a face cell of x
    and -inf on an edge cell of x0, K = 2."""
    x, x0 = lin_inputs(5, dtype, "specials", 2, nonfinite=False)
    x0[1, 1, 1], x[3, 3, 5], x0[5, 5, 2] = np.nan, np.inf, -np.inf
    return x, x0, 2


def project_inputs(N, dtype, K):
    """u, v, w (0.2-normal with a zero_region for K sweeps and -0 on one cell in sixteen) and u0, v0 to be overwritten."""
    rng = np.random.RandomState(3000 + N + K)
    f = {n: C.normal_field(N, dtype, 31 * N + q, 0.2) for q, n in enumerate(("u", "v", "w", "u0", "v0"))}
    f.update(C.zero_region({n: f[n] for n in ("u", "v", "w")}, max(K, 1), rng))
    hit = rng.random_sample(f["u"].shape) < 1.0 / 16.0
    for n in ("u", "v", "w"):
        f[n][hit] = -0.0
    return f


def advect_inputs(N, dtype, finite_velocity=False):
    """(d0, u, v, w): d0 with special values, mixed_flow with NaN, +-inf and +-0 planted, or (decomposed contexts, where
    a NaN in w is a reported halo violation) mixed_flow_one_plane as it is."""
    rng = np.random.RandomState(4000 + N)
    nf = nonfinite_at(N)
    d0 = specials(N, dtype, rng, N, nf)
    if finite_velocity:
        return (d0,) + tuple(C.mixed_flow_one_plane(N, dtype, N))
    return (d0,) + tuple(C.special_values(c, rng, nf) for c in C.mixed_flow(N, dtype, N))


def step_inputs(N, dtype, state):
    """The 8 named fields of a full-step case. "config1": zero but for config 1's source cell (docs/SPEC.md §5).
    "random": 0.2-normal fields and 0.03-normal velocities (one ghost plane suffices) with a zero_region, and two NaN:
    one in dens, one in dens0."""
    names = ("u", "v", "w", "u0", "v0", "w0", "dens", "dens0")
    if state == "config1":
        f = {n: np.zeros((N + 2,) * 3, dtype) for n in names}
        c = N // 2
        f["dens0"][c, c, c], f["v0"][c, c, c] = 100.0, 5.0
        return f
    rng = np.random.RandomState(5000 + N)
    f = {n: C.normal_field(N, dtype, 7 * N + q, 0.03 if n in ("u", "v", "w", "u0", "v0", "w0") else 0.2)
         for q, n in enumerate(names)}
    f = C.zero_region(f, STEP_K, rng)
    f["dens"][N, N, 1] = f["dens0"][1, 2, N] = np.nan
    return f


def tracer_inputs(N, dtype, exact=False):
    """(pos, fields, dt). exact (N = 16, dt = 0.125: dt0 = 2): uniform velocities of +-(k / 2) cells per call on
    tracers that start on integers and half-integers, so that p + dt0 * vel lands exactly on 0.5 and N + 0.5."""
    rng = np.random.RandomState(6000 + N)
    f = {n: C.normal_field(N, dtype, 11 * N + q, 0.5) for q, n in enumerate(("u", "v", "w", "dens"))}
    if not exact:
        return C.tracer_positions(N, dtype, N), f, DT
    for q, n in enumerate(("u", "v", "w")):
        f[n][...] = (-1.25, 0.75, 2.0)[q]  # dt0 * vel = -2.5, 1.5, 4 cells
    start = np.arange(0.5, N + 1.0, 0.5)
    pos = np.stack([start, start[::-1], start], axis=1).astype(dtype)
    return pos, f, C.LANDING_DT
