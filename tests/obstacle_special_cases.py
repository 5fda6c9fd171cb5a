"""The inputs, the case tables and the conditions that tests/test_obstacle_special_inputs_ref.py (CPU) and
tests/test_obstacle_special_gpu.py (device) share: the masked operators of docs/SPEC.md §15 to §17 on special values
that are operands - NaN, +-inf, zeros of either sign, subnormals, back-traces that land exactly on a cell centre - and
the three-field forms of the masked sweep and advect at every row shape. The fields come from tests/shape_cases.py and
tests/stable_cases.py, the masks from tests/obstacle_cases.py and tests/obstacle_mg_cases.py; what is added here is what
a mask asks of them: a solid cell hides what it holds, so every kind of special value is made to sit in a fluid cell
next to a solid one as well. Needs no GPU and no libsfgpu.so.

Every reference below takes `wrong` and `ops`, the wrong readings the numpy references can be switched to, so that the
CPU file runs the very case the GPU file compares under each of them."""
import numpy as np

import obstacle_cases as OC
import obstacle_mg_cases as MC
import obstacle_transport_cases as TC
import obstacle_transport_ref as TR
import obstacles_mg_ref as OM
import obstacles_ref as OB
import shape_cases as C
import stable_cases as SC
import stable_ref as S3
from gpu_support import DIFF, VISC, random_fields
from shape_cases import DT, dname

I = TR.I
F32, F64 = np.float32, np.float64
FAMILIES = ("specials", "zeros", "subnormal")
MASKS = {"specials": ("box", "random30", "walls"), "zeros": ("random30", "walls"), "subnormal": ("random30", "walls")}
SIZES = (5, 13, 34, 65, 70)  # 5: one ragged vector; 65, 70: the lane-64 / 65 seam of the flat advect, ragged tails
# (family, mask family, N, dtype) of the single-operator cases: b = 0 .. 3 each, one K per b
OPERATORS = [(f, m, N, t) for f in FAMILIES for m in MASKS[f] for N in SIZES for t in C.DTYPES]
LANDING = [(N, t) for N in (8, 64) for t in C.DTYPES]
SECOND_TRIP = [(131, F64), (262, F32)]  # the sweep, K = 1, walls, specials
DECOMPOSED = [(34, 2, "copy", F32), (34, 2, "rccl-self", F64)]
# sf_project_cg under a mask: (N, dtype, mask family), each velocity kind, none and jacobi:2
PROJECT_KINDS = ("zeros", "zero_region", "subnormal")
PROJECTIONS = [(13, F32, "random30"), (13, F64, "walls"), (34, F64, "random30"), (34, F32, "walls")]
PROJECT_ITERS, PROJECT_SWEEPS, CHECK_EVERY = 2, 2, 4
# sf_precondition_masked: (N, dtype, setting, mask family), r from each of CYCLE_KINDS
CYCLE_KINDS = ("zeros", "subnormal")
CYCLES = [(16, F32, MC.DEFAULT, "odd_box"), (16, F64, MC.SHORT, "random30"), (34, F64, MC.DEFAULT, "random30"),
          (34, F32, MC.SHORT, "odd_box")]
# vel_step + dens_step: plain CG, unbound sources
STEP_TOL, STEP_ITERS, STEP_K = 1e-2, 4, 2
STEPS = [(N, t) for N in (1, 2, 3, 5, 13, 34, 65, 70) for t in C.DTYPES]
BIG_STEPS = [(129, F64, "random30"), (131, F64, "walls"), (257, F32, "walls")]  # K = 1, max_iters = 1
_CACHE = {}


def once(key, build):
    """A reference computed once per key and only read afterwards."""
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def sweeps(N, b):
    """K of the sweep of field b at size N: 1, 2 and 4 all occur at every size."""
    return (1, 2, 4)[(N + b) % 3]


def operator_id(family, mfam, N, dtype):
    return f"{family}-{mfam}-N{N}-{dname(dtype)}"


def landing_id(N, dtype):
    return f"landing-N{N}-{dname(dtype)}"


def project_id(kind, N, dtype, mfam):
    return f"project-{kind}-{mfam}-N{N}-{dname(dtype)}"


def cycle_id(kind, N, dtype, s, mfam):
    return f"cycle-{kind}-" + MC.case_id(N, dtype, mfam, s)


def step_id(N, dtype):
    return f"step-N{N}-{dname(dtype)}"


def step_mask(N, dtype):
    return OC.mask("random30" if N % 2 else "walls", N, dtype)


# ---- what a mask asks of a field with special values ---------------------------------------------------------------
def is_kind(x, val):
    """Entries of x that hold val: NaN as NaN, zeros and infinities by their sign."""
    if np.isnan(val):
        return np.isnan(x)
    return (x == val) & (np.signbit(x) == np.signbit(val))


def kinds(nonfinite):
    return C.SPECIALS if nonfinite else C.SPECIALS[3:]


def closed_fluid(mask, axis=0):
    """Interior-shaped: fluid cells with a closed face, on the axis (1, 2, 3) if one is given."""
    mk = OB.Mask(mask)
    out = np.zeros(mk.solid.shape, bool)
    for face, closed in mk.closed.items():
        if axis == 0 or TR.AXIS[face] == axis:
            out |= closed
    return out & mk.fluid


def _ordinary(x):
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (x != 0)


def in_fluid(x, where, nonfinite):
    """A copy of x in which every kind of special value sits on a cell of `where` (interior-shaped) at least once: where
    none does, one planted value of the kind changes places with an ordinary value of such a cell."""
    x = x.copy()
    inner = x[I]
    for q, val in enumerate(kinds(nonfinite)):
        at = is_kind(inner, val)
        if (at & where).any():
            continue
        free = np.argwhere(where & _ordinary(inner))
        if not len(free):
            continue
        dst = tuple(free[(7919 * q + 13) % len(free)])
        src = np.argwhere(at)
        if len(src):
            inner[tuple(src[0])] = inner[dst]
        inner[dst] = val
    return x


def missing_kinds(x, where, nonfinite):
    return [val for val in kinds(nonfinite) if not (is_kind(x[I], val) & where).any()]


def seam_specials(x, rng):
    """A copy of x with every special value on cells 64 W and 64 W + 1 of a row (a row each): the last lane of a row
    kernel's first trip and the first of its second."""
    x = x.copy()
    N = x.shape[0] - 2
    s = 64 * (16 // x.dtype.itemsize)
    for val in C.SPECIALS:
        for i in (s, s + 1):
            x[1 + rng.randint(N), 1 + rng.randint(N), i] = val
    return x


def solid_sample(mask, vel, dt=DT, skip_first=False):
    """Interior-shaped: fluid cells of which at least one of the eight samples of advect_masked is solid (skip_first:
    one of the seven other than (i0, j0, k0)); and the weights (s1, t1, r1)."""
    N, T = mask.shape[0] - 2, mask.dtype.type
    solid = OB.solid_cells(mask)
    (i0, j0, k0), (x, y, z) = S3.SPEC.trace(vel, T(dt) * T(N))
    hit = np.zeros((N,) * 3, bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                if not (skip_first and di == dj == dk == 0):
                    hit |= solid[k0 + dk, j0 + dj, i0 + di]
    with np.errstate(invalid="ignore"):
        wts = x - i0.astype(T), y - j0.astype(T), z - k0.astype(T)
    return hit & OB.Mask(mask).fluid, wts


def own_operand(d0, hit, nonfinite):
    """A copy of d0 with -0 (and, with nonfinite, +inf and -inf) on a cell of `hit` each: for b = 0 the cell's own value
    is what stands in for its solid samples."""
    d0 = d0.copy()
    inner = d0[I]
    for q, val in enumerate((-0.0, np.inf, -np.inf) if nonfinite else (-0.0,)):
        if (is_kind(inner, val) & hit).any():
            continue
        free = np.argwhere(hit & _ordinary(inner))
        if len(free):
            inner[tuple(free[(104729 * q + 7) % len(free)])] = val
    return d0


def zeros_field(mask, axis):
    """-0 on every entry, shells included, and +0 on the fluid cells with a closed face on the axis (0: on any)."""
    x = np.full(mask.shape, -0.0, mask.dtype)
    x[I][closed_fluid(mask, axis)] = 0.0
    return x


def tiny_scale(dtype):
    return 4 * float(np.finfo(dtype).tiny)


# ---- the single operators ------------------------------------------------------------------------------------------
def sweep_inputs(family, mask, b, K):
    """(x, x0, non-finite values planted) of a sweep of field b under the mask."""
    N, dtype = mask.shape[0] - 2, mask.dtype.type
    if family == "zeros":
        return zeros_field(mask, b), np.full(mask.shape, -0.0, dtype), False
    x, x0 = SC.lin_inputs(N, dtype, family, K)
    if family == "subnormal":
        return x, x0, False
    nf = SC.nonfinite_at(N, K)
    if C.second_trip(N, dtype):
        rng = np.random.RandomState(8300 + N)
        x, x0 = seam_specials(x, rng), seam_specials(x0, rng)
    where = closed_fluid(mask)
    return in_fluid(x, where, nf), in_fluid(x0, where, nf), nf


def advect_inputs(family, mfam, mask, b, one_plane=False):
    """(d0, u, v, w, non-finite values planted)."""
    N, dtype = mask.shape[0] - 2, mask.dtype.type
    if family == "specials":
        d0, u, v, w = SC.advect_inputs(N, dtype, one_plane)
        nf = SC.nonfinite_at(N)
        d0 = in_fluid(d0, closed_fluid(mask), nf)
        return own_operand(d0, solid_sample(mask, (u, v, w))[0], nf), u, v, w, nf
    d0 = zeros_field(mask, b) if family == "zeros" else C.subnormal_field(N, dtype, 8000 + N)
    return (d0,) + tuple(TC.velocity(mfam, N, dtype, one_plane)) + (False,)


def run_sweep(family, mask, b, K, wrong=None, ops=S3.SPEC):
    x, x0, _ = sweep_inputs(family, mask, b, K)
    TR.diffuse_masked(b, x, x0, TC.DIFF, DT, K, mask, wrong, ops)
    return x


def run_advect(family, mfam, mask, b, wrong=None, ops=S3.SPEC, one_plane=False):
    d0, u, v, w, _ = advect_inputs(family, mfam, mask, b, one_plane)
    d = np.zeros_like(d0)
    TR.advect_masked(b, d, d0, u, v, w, DT, mask, wrong, ops=ops)
    return d


def operator_case(family, mfam, N, dtype, wrong=None, ops=S3.SPEC, P=None):
    """Every field the GPU case compares: {("sweep", b, K) | ("advect", b): the reference's result}."""
    def build():
        mask = OC.mask(mfam, N, dtype, P)
        out = {}
        for b in TC.BS:
            K = sweeps(N, b)
            out["sweep", b, K] = run_sweep(family, mask, b, K, wrong, ops)
            out["advect", b] = run_advect(family, mfam, mask, b, wrong, ops, P is not None)
        return out
    return once(("operators", family, mfam, N, dname(dtype), wrong, type(ops).__name__, P), build)


def second_trip_case(N, dtype, wrong=None, ops=S3.SPEC):
    """{("sweep", b, 1)}: walls, specials, K = 1; one b per size."""
    b = N % 4
    return {("sweep", b, 1): run_sweep("specials", OC.mask("walls", N, dtype), b, 1, wrong, ops)}


def across_the_boundary(x, mask, P):
    """A copy of x with every special value on a fluid cell of the last plane of the first slab and on one of the first
    plane of the second (fluid cells with a closed face where the plane has five)."""
    x = x.copy()
    N = x.shape[0] - 2
    fluid, near = OB.Mask(mask).fluid, closed_fluid(mask)
    for k in (N // P, N // P + 1):
        cells = np.argwhere(near[k - 1])
        if len(cells) < 5:
            cells = np.argwhere(fluid[k - 1])
        for q, val in enumerate(C.SPECIALS):
            j, i = cells[(q * len(cells)) // 5]
            x[k, 1 + j, 1 + i] = val
    return x


def decomposed_inputs(N, P, dtype):
    """walls with solid cells on both sides of the slab boundary; (mask, {b: (x, x0, K)}, {b: d0}, (u, v, w)): specials
    with finite velocities of at most one plane, a special value of every kind on each side of the boundary."""
    mask = OC.mask("walls", N, dtype, P)
    lin, adv = {}, {}
    for b in TC.BS:
        K = sweeps(N, b)
        x, x0, _ = sweep_inputs("specials", mask, b, K)
        lin[b] = (across_the_boundary(x, mask, P), across_the_boundary(x0, mask, P), K)
        d0, u, v, w, _ = advect_inputs("specials", "walls", mask, b, one_plane=True)
        adv[b] = across_the_boundary(d0, mask, P)
    return mask, lin, adv, (u, v, w)


def decomposed_case(N, P, dtype, wrong=None, ops=S3.SPEC):
    """The P = 1 reference of the decomposed case."""
    mask, lin, adv, vel = decomposed_inputs(N, P, dtype)
    out = {}
    for b in TC.BS:
        x, x0, K = lin[b]
        x = x.copy()
        TR.diffuse_masked(b, x, x0, TC.DIFF, DT, K, mask, wrong, ops)
        out["sweep", b, K] = x
        d = np.zeros_like(adv[b])
        TR.advect_masked(b, d, adv[b], *vel, DT, mask, wrong, ops=ops)
        out["advect", b] = d
    return out


# ---- exact landings under a mask -----------------------------------------------------------------------------------
LANDED = (np.inf, -np.inf, -0.0)


def landing_inputs(N, dtype):
    """(mask, d0, u, v, w, the three cells): C.exact_landing under random30 with dt = C.LANDING_DT, and d0 = +inf, -inf
    and -0 on three fluid cells whose trace lands exactly on a cell centre (s1 = t1 = r1 = 0) and which take a solid
    sample with weight zero: the zero weight multiplies wv = d0[c]. The +-inf cells come out NaN (0 * inf); the -0 cell
    comes out as the sample its trace lands on, plus products of weight zero whose signs the SPEC's sum decides."""
    mask = OC.mask("random30", N, dtype)
    d0, u, v, w = C.exact_landing(N, dtype, N, C.LANDING_DT)
    hit, (s1, t1, r1) = solid_sample(mask, (u, v, w), C.LANDING_DT, skip_first=True)
    cells = np.argwhere(hit & (s1 == 0) & (t1 == 0) & (r1 == 0) & _ordinary(d0[I]))
    chosen = [tuple(cells[(q * len(cells)) // 3]) for q in range(3)] if len(cells) >= 3 else []
    for c, val in zip(chosen, LANDED):
        d0[I][c] = val
    return mask, d0, u, v, w, chosen


def landing_case(N, dtype, wrong=None, ops=S3.SPEC):
    mask, d0, u, v, w, _ = landing_inputs(N, dtype)
    d = np.zeros_like(d0)
    TR.advect_masked(0, d, d0, u, v, w, C.LANDING_DT, mask, wrong, ops=ops)
    return {("advect", 0): d}


# ---- the projection and the masked V-cycle -------------------------------------------------------------------------
def project_velocity(kind, mask):
    N, dtype = mask.shape[0] - 2, mask.dtype.type
    if kind == "zeros":
        return [zeros_field(mask, axis) for axis in (1, 2, 3)]
    if kind == "zero_region":
        f = SC.project_inputs(N, dtype, PROJECT_ITERS)
        return [f[n] for n in ("u", "v", "w")]
    return [C.subnormal_field(N, dtype, 8100 + N + q, scale=tiny_scale(dtype)) for q in range(3)]


def project_case(kind, N, dtype, mfam, m, wrong=None, ops=S3.SPEC):
    """OB.project_cg of the case, two iterations at most, m Jacobi sweeps as the preconditioner."""
    def build():
        mask = OC.mask(mfam, N, dtype)
        return OB.project_cg(*project_velocity(kind, mask), mask, OC.TOL, PROJECT_ITERS, m, wrong=wrong, ops=ops)
    return once(("project", kind, N, dname(dtype), mfam, m, wrong, type(ops).__name__), build)


def cycle_rhs(kind, mask):
    N, dtype = mask.shape[0] - 2, mask.dtype.type
    return zeros_field(mask, 0) if kind == "zeros" else C.subnormal_field(N, dtype, 8200 + N, scale=tiny_scale(dtype))


def cycle_case(kind, N, dtype, s, mfam, wrong=None):
    mask = MC.mask(mfam, N, dtype)
    return OM.vcycle(cycle_rhs(kind, mask)[I], mask, *s, wrong=wrong)


# ---- the steps -----------------------------------------------------------------------------------------------------
def step_fields(N, dtype):
    return random_fields(N, dtype, 190 + N)


def step_case(N, dtype, wrong=None, ops=S3.SPEC):
    """One vel_step + dens_step composed from the references: (the second projection's outcome, the density)."""
    def build():
        f = step_fields(N, dtype)
        mask = step_mask(N, dtype)
        project = lambda u, v, w: OB.project_cg(u, v, w, mask, STEP_TOL, STEP_ITERS, 0, wrong=wrong, ops=ops)  # noqa: E731
        vel = TR.vel_step(f, mask, STEP_K, DT, VISC, project, wrong=wrong, ops=ops)
        dens = TR.dens_step(f["dens"], f["dens0"], vel["u"], vel["v"], vel["w"], mask, STEP_K, DT, DIFF, wrong=wrong, ops=ops)
        return vel, dens
    return once(("step", N, dname(dtype), wrong, type(ops).__name__), build)


def big_step_fields(N, dtype, seed):
    """The fields of gpu_support.random_fields drawn in the dtype (a 257^3 step draws 136 million numbers)."""
    rng = np.random.default_rng(seed)
    names = ("u", "v", "w", "u0", "v0", "w0", "dens", "dens0")
    scale = {n: dtype(0.05 if n in ("u", "v", "w") else 0.2) for n in names}
    return {n: scale[n] * rng.standard_normal((N + 2,) * 3, dtype=dtype) for n in names}


# ---- the condition on every compared field -------------------------------------------------------------------------
def check_nan_share(fields, mask, what):
    """stable_cases.check_nan_share on the fluid cells (a solid cell is +0 by rule): a comparison says little once NaN
    has spread, so fewer than a quarter of the fluid interior cells of every compared field of the reference are NaN.
    Returns the largest share."""
    fluid = OB.Mask(mask).fluid
    worst = 0.0
    for n, x in fields.items():
        share = float(np.isnan(x[I][fluid]).mean()) if fluid.any() else 0.0
        assert share < 0.25, f"{what}: {n}: NaN on {share:.3f} of the reference's fluid cells: the case is vacuous"
        worst = max(worst, share)
    return worst
