"""The cases of the multigrid-preconditioner tests (docs/SPEC.md §11.3), shared by tests/test_pressure_mg_gpu.py, which
runs them on the device, and tests/test_pressure_mg_ref.py, which shows on the CPU which wrong V-cycle each of them
tells from the right one. Importing this module needs no GPU and no libsfgpu.so."""
import numpy as np

import pressure_mg_ref as G
import shape_cases as C
import stable_ref as S3
from gpu_support import DT, VISC

TOL = 1e-3
DEFAULT = (2, 0, 8)  # (nu, max_levels, nu_c)
SETTINGS = [(1, 0, 1), (2, 0, 8), (3, 2, 4), (2, 1, 8)]
NO_COARSENING = [1, 2, 3, 5, 6, 7, 13]           # odd, or n / 2 < 4: nu_c sweeps on the fine grid
HIERARCHIES = [8, 12, 16, 24, 34, 36, 40, 64, 70]  # every shape of hierarchy: depth 2 to 5, odd and even coarsest levels
SIZES = NO_COARSENING + HIERARCHIES
# a fine row takes a second trip (more than 64 vectors of 16 bytes): with DEFAULT only
SECOND_TRIP = [(130, np.float64), (132, np.float64), (260, np.float32), (264, np.float32)]
TO_CONVERGENCE = 400  # a limit no run reaches
LONG_ITERS = 2        # max_iters at the second-trip sizes of the solve cases: the numpy side stays under a minute
SOLVE_SIZES = SIZES
LONG_SOLVES = [(130, np.float64), (260, np.float32)]
# (N, P, transport, max_levels): every coarse level splits into whole planes per slab
DECOMPOSED = [(64, 2, "copy", 0), (64, 4, "rccl-self", 0), (34, 17, "rccl-self", 0), (72, 3, "copy", 0),
              (40, 2, "copy", 3), (64, 8, "copy", 4)]
DECOMPOSED_ITERS = 6
REJECTED = [(40, 2, 3), (64, 8, 4)]  # (N, P, the largest admissible max_levels) at max_levels = 0

# Seeds of the right-hand sides of the sf_precondition cases: 700 + N unless another one is needed for a case to tell a
# mutant of tests/test_pressure_mg_ref.py from the reference in bits.
SEEDS = {}


def seed(N):
    return SEEDS.get(N, 700 + N)


def setting_id(s):
    return "nu%d-L%d-c%d" % s


def case_id(N, dtype, s=DEFAULT, P=1):
    """The id of a case of the GPU file's tests of sf_precondition, as pytest prints it."""
    return f"N{N}-{C.dname(dtype)}-{setting_id(s)}" + (f"-P{P}" if P > 1 else "")


def precondition_fields(N, dtype, sd=None):
    """(z0, r): standard normal on all (N+2)^3 entries, no set_bnd: whatever z held and the shells of r are independent
    random numbers that a correct z = M(r) never shows."""
    rng = np.random.RandomState(seed(N) if sd is None else sd)
    return tuple(rng.standard_normal((N + 2,) * 3).astype(dtype) for _ in range(2))


def reference_vel_step(f, K, tol, max_iters, mg):
    """SPEC §3 vel_step on copies of the velocity fields of f, both projections pressure_mg_ref.project_cg with the
    setting mg (no bound sources, no forces, semi-Lagrangian advection). Returns the second projection's outcome."""
    u, v, w, u0, v0, w0 = (f[n].copy() for n in ("u", "v", "w", "u0", "v0", "w0"))
    T = u.dtype.type
    Nf = T(u.shape[0] - 2)
    for x, s in ((u, u0), (v, v0), (w, w0)):
        S3.add_source(x, s, DT)
    u, u0, v, v0, w, w0 = u0, u, v0, v, w0, w
    a = ((T(DT) * T(VISC)) * Nf) * Nf
    for b, x, x0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        S3.lin_solve(b, x, x0, a, T(1) + T(6) * a, K)
    out = G.project_cg(u, v, w, tol, max_iters, *mg)
    u0, v0, w0 = out["u"], out["v"], out["w"]
    u, v, w = (np.zeros_like(u0) for _ in range(3))
    for b, d, d0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        S3.advect(b, d, d0, u0, v0, w0, DT)
    return G.project_cg(u, v, w, tol, max_iters, *mg)
