"""The case table shared by tests/test_pressure_pcg_ref.py (CPU: the inputs discriminate) and
tests/test_pressure_pcg_gpu.py (GPU: the preconditioned CG projection of SPEC §11.2 against tests/pressure_pcg_ref.py).
The inputs are shape_cases.cg_velocity; sizes and decompositions are those of shape_cases. PLANS (below) is the table of
tests/test_pressure_pcg_plans_gpu.py: one case per pass plan that z = M(r) can run as, on one slab and on slabs."""
import numpy as np

import shape_cases as C

TOL = 1e-3
M = 4                       # the sweep count of the shape and decomposition cases
SWEEPS = [1, 2, 3, 4, 5, 8]  # one sweep (a really zeroed z), a pair, a pair and a single, ..., two marching passes
SWEEP_SIZES = [34, 65]
ROW_SHAPES = ([(N, t) for N in (1, 2, 3, 5, 13, 31, 34, 64, 65, 70, 130) for t in C.DTYPES]
              + [(N, np.float64) for N in (128, 129, 131, 200)] + [(N, np.float32) for N in (256, 257, 262, 324)])
TO_CONVERGENCE = 400        # a limit no run below N = 128 reaches
DECOMPOSED_ITERS = 6

# Seeds: shape_cases.cg_seed(N), except where another seed makes a sum r.z of the run differ between the §10 order and a
# second trip added to lane 0 cell by cell (tests/test_pressure_pcg_ref.py: at N = 131 in fp64 the gamma' of the first
# iteration).
SEEDS = {131: 3}


def seed(N):
    return SEEDS.get(N, C.cg_seed(N))


def max_iters(N):
    """To convergence below N = 128; six iterations from there up (the numpy reference of a case stays at a minute)."""
    return TO_CONVERGENCE if N < 128 else 6


# ---- the pass plans of z = M(r) ----------------------------------------------------------------------------------------
# M(r) is op_lin_solve, so which kernels, ghost depths and trapezoid blocks a preconditioned solve runs is decided by
# Solver::plan_solve. A plan is written as the sweep counts of its passes: `Z` marks a first pass on the implicit zero
# iterate, `C` one that reads the stored (memset) z, `+e` the trapezoid growth Pass::extra of the boundary launch.
# model() is plan_solve, pass_sweeps, the choice of G and can_fuse2 of sf_solver.hpp said again in Python; the GPU file
# reads every case's plan back from its schedule trace (gpu_support.traced_plans), so the table states what really ran.
MARCH = {"SF_MARCH_MINCELLS_K": "0"}               # the marching kernel takes grids of any size
MARCH_MINP4 = dict(MARCH, SF_MARCH_MINP="4")       # ... and plane ranges from four planes up (default 12)


def model(N, dtype, P, m, env=None, transport="copy", trap=None):
    """(G, plan) of the m-sweep solve of op_precondition on a context created under `env`. trap: the trapezoid depth
    where neither SF_TRAP nor the transport's default decides it (an rccl-self context measures it: tune_schedule)."""
    env = env or {}

    def sw(name, default):
        return int(env.get(name, default))

    W = 16 // np.dtype(dtype).itemsize
    ghost, sk_s, minp = sw("SF_GHOST", 4), sw("SF_SK_S", 4), sw("SF_MARCH_MINP", 12)
    sk_first, fuse2, split = sw("SF_SK_FIRST", 1) != 0, sw("SF_FUSE2", 1) != 0, sw("SF_SPLIT", 1) != 0
    ishell, march, zero_skip = sw("SF_ISHELL", 1) != 0, sw("SF_MARCH", 1) != 0, sw("SF_ZERO_SKIP", 1) != 0
    mincells = sw("SF_MARCH_MINCELLS_K", 2500) * 1000
    if "SF_TRAP" in env:
        trap = int(env["SF_TRAP"])
    elif trap is None:
        trap = 0 if (transport == "rccl-self" and P > 1) else 5
    nzl = N // P
    fusable = fuse2 and N % W == 0 and N // W <= 512

    def march_fits(planes):
        return march and planes >= minp and N * N * planes >= mincells

    G = 2 if (P > 1 and nzl >= 2 and fusable and ghost >= 2) else 1
    for gs in (3, 4):
        if G == gs - 1 and ghost >= gs and sk_s >= gs and split and march_fits(nzl - 2 * gs):
            G = gs
    can_fuse2 = fusable and (P == 1 or G >= 2)

    def march_takes(planes):
        return ishell and march_fits(planes)

    def march_pass(S, extra=0):
        if P == 1:
            return march_takes(nzl)
        return G >= S and split and march_takes(nzl - 2 * (max(S, G) + extra))

    def pass_sweeps(it, first, extra):
        pair, left = can_fuse2 and it + 2 <= m, m - it
        if first:
            return 4 if (sk_first and sk_s >= 4 and can_fuse2 and m >= 7 and march_pass(4)) else 2 if pair else 1
        marching = pair and sk_s >= 3 and left >= 3
        if marching and sk_s >= 4 and left >= 4 and left not in (5, 6) and march_pass(4, extra):
            return 4
        if marching and left != 4 and march_pass(3, extra):
            return 3
        return 2 if pair else 1

    x_zero = can_fuse2 and m >= 2 and zero_skip
    out, tj, dprev, sprev, it = [], 0, 0, 0, 0
    while it < m:
        pair = can_fuse2 and it + 2 <= m
        s = pass_sweeps(it, it == 0, 0)
        depth0 = max((4 if G >= 3 else 2) if s == 2 else s, G)
        d = dprev + max(s, sprev)
        cont = pair and P > 1 and G >= 2 and trap > 1 and 0 < tj < trap and d >= depth0 and nzl > 2 * d + 2
        if cont and s >= 3 and pass_sweeps(it, it == 0, d - depth0) != s:
            cont = False
        if cont and s == 2 and d & 1:
            cont = False
        extra = d - depth0 if cont else 0
        first = "" if it else ("Z" if x_zero and pair else "C")
        shown = extra if split else 0  # (without the two-stream schedule for_planes launches no deeper boundary)
        out.append(f"{s}{first}" + (f"+{shown}" if shown else ""))
        dprev, sprev, tj = depth0 + extra, s, (tj + 1 if cont else 1)
        it += s
    return G, " ".join(out)


def parse_plan(plan):
    """[(sweeps, first, extra)] of a plan string: first is "Z", "C" or "" (not a first pass)."""
    out = []
    for tok in plan.split():
        body, _, extra = tok.partition("+")
        first = body[-1] if body[-1] in "ZC" else ""
        out.append((int(body.rstrip("ZC")), first, int(extra or 0)))
    return out


class Plan:
    """One case: project_cg with jacobi:m at (N, dtype) on P slabs over `transport`, created under `env`; `G` ghost
    planes and pass plan `plan`. tuned: an rccl-self context without SF_TRAP, whose trapezoid depth (0, 2 or 5) is
    measured when it is created; its plan is model(..., trap=<the depth the context reports>)."""

    def __init__(self, N, dtype, P, transport, env, m, tuned=False):
        self.N, self.dtype, self.P, self.transport, self.env, self.m, self.tuned = N, dtype, P, transport, dict(env), m, tuned
        self.G, self.plan = model(N, dtype, P, m, env, transport)

    def plan_at(self, trap):
        return model(self.N, self.dtype, self.P, self.m, self.env, self.transport, trap=trap)

    @property
    def id(self):
        sw = ",".join(f"{k[3:]}={v}" for k, v in self.env.items() if k != "SF_MARCH_MINCELLS_K")
        return f"N{self.N}-{C.dname(self.dtype)}-P{self.P}-{self.transport}-m{self.m}" + (f"-{sw}" if sw else "") + (
            "-untuned" if self.tuned else "")


PLAN_SWEEPS = [2, 5, 6, 7, 8, 9, 10, 11, 12]
SLAB_SWEEPS = [5, 7, 8, 9, 10, 11, 12]
NO_SKIP = dict(MARCH, SF_ZERO_SKIP="0")  # z is memset and the first pass, a marching one too, reads the stored zeros


def _plans():
    out = []
    for dtype in C.DTYPES:
        # one slab: every pass plan of 2 .. 12 sweeps, m = 3 and m = 1 for the single sweep, the stored zero
        for N in (40, 64):
            out += [Plan(N, dtype, 1, "copy", MARCH, m) for m in PLAN_SWEEPS]
        out += [Plan(40, dtype, 1, "copy", MARCH, 3), Plan(40, dtype, 1, "copy", MARCH, 1),
                Plan(40, dtype, 1, "copy", NO_SKIP, 8), Plan(64, dtype, 1, "copy", NO_SKIP, 5)]
        # slabs; copy and rccl-self alternate, and an rccl-self case that is there for growth sets SF_TRAP=5
        slabs = []
        slabs += [(72, 2, MARCH, m) for m in SLAB_SWEEPS]                      # the full trapezoid at the default MINP
        slabs += [(64, 2, MARCH if m <= 9 else MARCH_MINP4, m) for m in SLAB_SWEEPS]
        slabs += [(40, 2, MARCH, m) for m in [3] + SLAB_SWEEPS]                # interior exactly MINP long: no growth
        slabs += [(72, 3, MARCH_MINP4, m) for m in (7, 8, 10, 12)]            # three slabs, growth on the second pass
        slabs += [(64, 4, MARCH, m) for m in (8, 9, 12)]                        # G = 2: long pair trapezoids
        slabs += [(40, 2, NO_SKIP, 8), (72, 2, NO_SKIP, 5)]
        for n, (N, P, env, m) in enumerate(slabs):
            transport = ("copy", "rccl-self")[n % 2]
            grows = "+" in model(N, dtype, P, m, env, "copy")[1]
            if transport == "rccl-self" and grows:
                env = dict(env, SF_TRAP="5")
            out.append(Plan(N, dtype, P, transport, env, m))
        out.append(Plan(72, dtype, 2, "rccl-self", MARCH, 8, tuned=True))
    return out


PLANS = _plans()
ONE_SLAB = [c for c in PLANS if c.P == 1]
ON_SLABS = [c for c in PLANS if c.P > 1]
CONVERGED_M = 8  # one run to convergence per (N, P) of ON_SLABS at this m
