"""The numpy statement of the multigrid preconditioner (docs/SPEC.md §11.3, tests/pressure_mg_ref.py) on the CPU: the
level table, the first sweep, the symmetry of M, the iteration counts the feature exists for, and which case of
tests/test_pressure_mg_gpu.py tells each wrong V-cycle from the right one in bits. No GPU needed."""
import numpy as np
import pytest

import mg_cases as MC
import pressure_cg_ref as R
import pressure_mg_ref as G
import pressure_pcg_ref as Q
import shape_cases as C
from ref_support import same_bits

I = R.I
F32, F64 = np.float32, np.float64

# ---- the level table ---------------------------------------------------------------------------------------------------
LEVELS = {1: [1], 2: [2], 3: [3], 4: [4], 5: [5], 6: [6], 7: [7], 8: [8, 4], 12: [12, 6], 16: [16, 8, 4], 24: [24, 12, 6],
          34: [34, 17], 36: [36, 18, 9], 40: [40, 20, 10, 5], 64: [64, 32, 16, 8, 4], 70: [70, 35], 72: [72, 36, 18, 9],
          130: [130, 65], 256: [256, 128, 64, 32, 16, 8, 4], 260: [260, 130, 65], 264: [264, 132, 66, 33]}


@pytest.mark.parametrize("N", sorted(LEVELS))
def test_level_table(N):
    full = LEVELS[N]
    assert G.levels(N) == G.levels(N, 0) == full
    for max_levels in (1, 2, 3):
        assert G.levels(N, max_levels) == full[:max_levels]
    # the rule itself: halve while even and the half is at least 4
    for a, b in zip(full, full[1:]):
        assert a % 2 == 0 and b == a // 2 and b >= 4
    assert full[-1] % 2 == 1 or full[-1] // 2 < 4


def test_admissible_depths_of_the_issue():
    assert G.admissible_levels(64, 4) == 5 and G.admissible_levels(64, 8) == 4
    assert G.admissible_levels(40, 2) == 3 and G.admissible_levels(34, 17) == 2
    assert G.admissible_levels(72, 3) == 4
    for N, P, want in MC.REJECTED:
        assert G.admissible_levels(N, P) == want < len(G.levels(N))
    for N, P, _, max_levels in MC.DECOMPOSED:
        assert len(G.levels(N, max_levels)) <= G.admissible_levels(N, P)


# ---- the first sweep ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
def test_first_sweep_is_zero_plus_cs_r(dtype):
    """One sweep from z = +0 is T(0) + c_s r in bits: where r is -0 (or c_s r underflows to -0) the result is +0."""
    rng = np.random.RandomState(3)
    r = rng.standard_normal((7, 7, 7)).astype(dtype)
    r[1, 2, 3], r[0, 0, 0], r[6, 6, 6] = -0.0, 0.0, -np.finfo(dtype).tiny * dtype(1e-30)
    r[2, 2, 2] = -np.finfo(dtype).smallest_subnormal
    zero = np.zeros((9, 9, 9), dtype)
    got, want = G.smooth(zero, r), G.first_sweep(r)
    assert same_bits(got, want)
    assert not np.signbit(got[2, 3, 4]) and not np.signbit(got[3, 3, 3]) and got[3, 3, 3] == 0
    assert same_bits(G.vcycle(r, 1, 1, 1), want)  # no coarsening, nu_c = 1: the cycle is that sweep
    # c_s r alone would keep the sign
    assert np.signbit((dtype(1.0 / 7.0) * r)[1, 2, 3])


# ---- symmetry ----------------------------------------------------------------------------------------------------------
def _asym(N, variant=None, seed=0):
    rng = np.random.RandomState(100 + N + seed)
    x, y = rng.standard_normal((2, N, N, N))
    Mx = G.vcycle(x, 2, 0, 8, variant)[I, I, I]
    My = G.vcycle(y, 2, 0, 8, variant)[I, I, I]
    return abs(np.sum(x * My) - np.sum(y * Mx)) / (np.linalg.norm(x) * np.linalg.norm(My))


@pytest.mark.parametrize("N", [8, 12, 16])
def test_M_is_symmetric(N):
    """|x.M y - y.M x| <= 1e-10 |x| |M y| in fp64 (M is symmetric in exact arithmetic; about 1e4 operations per cell times
    2^-53, with margin); a cycle with nu + 1 post-sweeps is not symmetric, and is seen beyond 1e-6."""
    a, b = _asym(N), _asym(N, "extra_post_sweep")
    print(f"N={N}: asymmetry {a:.3e}, with one more post-sweep {b:.3e}")
    assert a <= 1e-10
    assert b > 1e-6


@pytest.mark.parametrize("N", [8, 12, 16])
def test_M_is_positive_on_mean_free_vectors(N):
    rng = np.random.RandomState(N)
    for _ in range(3):
        x = rng.standard_normal((N, N, N))
        x -= x.mean()
        assert np.sum(x * G.vcycle(x, 2, 0, 8)[I, I, I]) > 0


# ---- iteration counts --------------------------------------------------------------------------------------------------
def test_iteration_counts_do_not_grow_with_N():
    """On shape_cases.cg_velocity at tol = 1e-3: at N = 64 the V-cycle (2, 0, 8) takes fewer than half the iterations of
    the Jacobi sweeps with m = 8, and no more than two more than at N = 32."""
    its = {}
    for N in (32, 64):
        vel = C.cg_velocity(N, F32, C.cg_seed(N))
        its[N] = G.project_cg(*vel, MC.TOL, MC.TO_CONVERGENCE, *MC.DEFAULT)
        assert its[N]["status"] == G.CONVERGED
    jac = Q.project_cg(*C.cg_velocity(64, F32, C.cg_seed(64)), MC.TOL, MC.TO_CONVERGENCE, 8)
    print(f"V-cycle: {its[32]['iterations']} at 32, {its[64]['iterations']} at 64; jacobi:8 at 64: {jac['iterations']}")
    assert jac["status"] == G.CONVERGED
    assert 2 * its[64]["iterations"] < jac["iterations"]
    assert its[64]["iterations"] <= its[32]["iterations"] + 2


def test_capped_hierarchies_converge_more_slowly():
    vel = C.cg_velocity(32, F32, C.cg_seed(32))
    full, two = (G.project_cg(*vel, MC.TOL, MC.TO_CONVERGENCE, 2, L, 8)["iterations"] for L in (0, 2))
    assert full < two


# ---- mutants: the GPU case whose inputs tell each from the reference ----------------------------------------------------
# variant -> (N, dtype, setting): a case of test_pressure_mg_gpu.py::test_precondition (mg_cases.case_id)
MUTANT_CASES = {
    "restrict_assoc": (8, F32, (2, 0, 8)),
    "quarter": (8, F64, (2, 0, 8)),
    "parent_floor": (12, F32, (2, 0, 8)),
    "no_bnd_after_prolong": (8, F32, (1, 0, 1)),
    "coarse_as_nu": (16, F64, (2, 0, 8)),
    "coarsen_to_2": (6, F32, (2, 0, 8)),
}


@pytest.mark.parametrize("variant", sorted(MUTANT_CASES), ids=[f"{v}-seen-by-{MC.case_id(*MUTANT_CASES[v])}"
                                                               for v in sorted(MUTANT_CASES)])
def test_a_gpu_case_tells_the_mutant(variant):
    N, dtype, s = MUTANT_CASES[variant]
    assert N in MC.SIZES and s in MC.SETTINGS and variant in G.VARIANTS
    _, r = MC.precondition_fields(N, dtype)
    want = G.vcycle(r[I, I, I], *s)
    assert not same_bits(G.vcycle(r[I, I, I], *s, variant=variant), want)
    assert same_bits(G.vcycle(r[I, I, I].copy(), *s), want)


def test_coarsening_to_two_also_shows_below_a_real_hierarchy():
    """n / 2 >= 2 in place of >= 4 adds a level under 12 -> 6 as well."""
    _, r = MC.precondition_fields(12, F64)
    assert not same_bits(G.vcycle(r[I, I, I], 2, 0, 8, "coarsen_to_2"), G.vcycle(r[I, I, I], 2, 0, 8))


@pytest.mark.parametrize("N,dtype", [(5, F32), (8, F64), (34, F32)],
                         ids=[f"seen-by-two-calls-{MC.case_id(n, t)}" for n, t in [(5, F32), (8, F64), (34, F32)]])
def test_two_calls_tell_a_z_that_is_not_zeroed(N, dtype):
    """The second of two calls (test_precondition repeats every call) starts from the first one's z in the mutant."""
    _, r = MC.precondition_fields(N, dtype)
    want = G.vcycle(r[I, I, I], *MC.DEFAULT)
    assert not same_bits(G.vcycle(r[I, I, I], *MC.DEFAULT, z_init=want), want)
    # ... and the first call from whatever the slot held
    z0, _ = MC.precondition_fields(N, dtype)
    assert not same_bits(G.vcycle(r[I, I, I], *MC.DEFAULT, z_init=z0), want)


STALE = [(N, P, L) for N, P, _, L in MC.DECOMPOSED]


@pytest.mark.parametrize("N,P,L", STALE, ids=[f"seen-by-{MC.case_id(n, F32, (2, l, 8), p)}" for n, p, l in STALE])
def test_decomposed_cases_tell_stale_ghost_planes_after_the_correction(N, P, L):
    """Slab emulation: the first post-sweep of every level reads z beyond the slab as it was before step 5. With every
    plane current the emulation is the reference."""
    _, r = MC.precondition_fields(N, F32)
    s = (2, L, 8)
    want = G.vcycle(r[I, I, I], *s)
    assert not same_bits(G.vcycle(r[I, I, I], *s, variant="stale_after_prolong", slabs=P), want)
    assert same_bits(G.vcycle(r[I, I, I], *s, variant="stale_after_prolong", slabs=1), want)


def test_project_cg_with_the_jacobi_M_is_the_reference_of_11_2():
    """The iteration around M is §11.2's: with M = pressure_pcg_ref.precondition it leaves that module's bits."""
    vel = C.cg_velocity(13, F64, C.cg_seed(13))
    a = G.project_cg(*vel, MC.TOL, 6, 0, M=lambda r: Q.precondition(r, 4))
    b = Q.project_cg(*vel, MC.TOL, 6, 4)
    assert (a["status"], a["iterations"], a["rel_residual"]) == (b["status"], b["iterations"], b["rel_residual"])
    for n in ("u", "v", "w", "p", "div"):
        assert same_bits(a[n], b[n])
