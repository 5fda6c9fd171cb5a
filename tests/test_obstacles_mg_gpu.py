"""Obstacle-aware multigrid on the device (docs/SPEC.md §16: sf_set_obstacle_multigrid, sf_precondition_masked): everything
is held to the bits of tests/obstacles_mg_ref.py on the masks of tests/obstacle_mg_cases.py.

(a) sf_precondition_masked against vcycle at every shape of hierarchy, the last-lane and second-trip sizes included; r
    holds a NaN in every solid cell for a second call;
(b) sf_project_cg under a mask with the V-cycle in force, check_every 0 and 4; two vel_step + dens_step;
(c) the admissible decompositions over both transports;
(d) the setting: off still refuses, on then obstacles off is §11.3, a second mask and another max_levels are honoured,
    an unmasked cycle issues no masked launch.
tests/test_obstacles_mg_ref.py shows on the CPU which wrong readings of §16 these cases tell from the right one. The
schedule-hazard check of tests/conftest.py reads the trace of every context created here."""
import os
import time

import numpy as np
import pytest

import diagnostics_ref as D
import obstacle_mg_cases as MC
import obstacles_mg_ref as OM
import obstacles_ref as OB
import pressure_mg_ref as G
import shape_cases as C
from gpu_support import DIFF, DT, VISC, S, assert_same_bits, make, random_fields, slab0_ops, upload_all

pytestmark = pytest.mark.gpu

I = OM.I
OUT = (("u", "u"), ("v", "v"), ("w", "w"), ("u0", "p"), ("v0", "div"))
MASK_SLOT = "dens0"  # a slot neither the projection nor sf_precondition_masked touches
_CYCLES, _SOLVES = {}, {}


def want_cycle(family, N, dtype, s, P=None):
    """vcycle of the case's mask and right-hand side: computed once per case, only read afterwards."""
    key = (family, N, C.dname(dtype), s, P)
    if key not in _CYCLES:
        t0 = time.perf_counter()
        _, r = MC.rhs_fields(family, N, dtype)
        _CYCLES[key] = OM.vcycle(r[I, I, I], MC.mask(family, N, dtype, P), *s)
        print(f"vcycle {key}: {time.perf_counter() - t0:.1f} s")
    return _CYCLES[key]


def want_solve(family, N, dtype, iters, s, P=None):
    key = (family, N, C.dname(dtype), iters, s, P)
    if key not in _SOLVES:
        t0 = time.perf_counter()
        _SOLVES[key] = OM.project_cg(*MC.velocity(family, N, dtype), MC.mask(family, N, dtype, P), MC.TOL, iters, *s)
        print(f"project_cg {key}: {time.perf_counter() - t0:.1f} s")
    return _SOLVES[key]


def masked_multigrid(fs, mask, s, slot=MASK_SLOT):
    """Obstacles, the V-cycle and the setting of §16, in that order."""
    fs.set_obstacles(mask, slot=slot)
    fs.fill(slot, float("nan"))  # the mask is read once
    fs.set_pressure_multigrid(*s)
    assert fs.obstacle_multigrid() is False
    fs.set_obstacle_multigrid(True)
    assert fs.obstacle_multigrid() is True


def check_cycle(fs, family, N, dtype, want, what, parked=True):
    """z and r uploaded with independent random shells; z = V_m(0, r) whole against the reference, then once more with
    a NaN in every solid cell of r and in all of z."""
    z0, r = MC.rhs_fields(family, N, dtype)
    fs.upload("u0", z0)
    fs.upload("v0", r)
    fs.precondition_masked("u0", "v0")
    fs.sync()
    assert_same_bits(fs.download("u0"), want, f"{what}: z")
    assert_same_bits(fs.download("v0"), r, f"{what}: r is left alone")
    if parked:
        solid = OB.Mask(MC.mask(family, N, dtype)).solid
        fs.upload("v0", parked_nan(r, solid))
        fs.fill("u0", float("nan"))
        fs.precondition_masked("u0", "v0")
        fs.sync()
        assert_same_bits(fs.download("u0"), want, f"{what}: z with NaN in the solid cells of r")


def parked_nan(x, solid):
    x = x.copy()
    x[I, I, I][solid] = np.nan
    return x


def check_solve(fs, family, N, dtype, iters, want, what):
    mask = MC.mask(family, N, dtype)
    for n, a in zip(("u", "v", "w"), MC.velocity(family, N, dtype)):
        fs.upload(n, a)
    info = fs.project_cg("u", "v", "w", "u0", "v0", MC.TOL, iters)
    fs.sync()
    print(f"{what}: got {info} want status {want['status']} iterations {want['iterations']} rel {want['rel_residual']!r}")
    assert (info["status"], info["iterations"]) == (want["status"], want["iterations"]), what
    assert D.bits(info["rel_residual"]) == D.bits(want["rel_residual"]), what
    for slot, name in OUT:
        assert_same_bits(fs.download(slot), want[name], f"{what}: {name}")
    got = fs.poisson_residual("u0", "v0")
    assert D.bits(got) == D.bits(OB.poisson_residual(want["p"], want["div"], mask)), what


# ---- (a) -----------------------------------------------------------------------------------------------------------
CYCLES = [(N, t, s, f) for N, t, s, fams in MC.PRECONDITION for f in fams]


@pytest.mark.parametrize("N,dtype,s,family", CYCLES, ids=[MC.case_id(n, t, f, s) for n, t, s, f in CYCLES])
def test_precondition_masked(N, dtype, s, family):
    want = want_cycle(family, N, dtype, s)
    with make(N, dtype) as fs:
        masked_multigrid(fs, MC.mask(family, N, dtype), s)
        assert fs.pressure_multigrid["levels"] == len(G.levels(N, s[1]))
        check_cycle(fs, family, N, dtype, want, MC.case_id(N, dtype, family, s))


# ---- (b) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype,family", MC.SOLVES, ids=[f"{f}-N{n}-{C.dname(t)}" for n, t, f in MC.SOLVES])
def test_project_cg_under_a_mask(N, dtype, family):
    """Eight iterations at most with (2, 0, 8), the scalars on the host and on the device."""
    want = want_solve(family, N, dtype, MC.ITERS, MC.DEFAULT)
    assert want["iterations"] >= 1
    with make(N, dtype) as fs:
        masked_multigrid(fs, MC.mask(family, N, dtype), MC.DEFAULT)
        for every in (0, MC.CHECK_EVERY):
            fs.set_pressure_sync(every)
            check_solve(fs, family, N, dtype, MC.ITERS, want, f"{family} N={N} {C.dname(dtype)} sync={every}")


STEP_TOL, STEP_MG = 1e-2, (2, 3, 8)  # (40, 20, 10: the depth two slabs admit)
_STEPS = {}


def step_reference(N, f, mask):
    """Two vel_step + dens_step composed from the references; computed once per size."""
    if N not in _STEPS:
        g, outs = dict(f), []
        for _ in range(2):
            vel = OM.vel_step(g, mask, MC.STEP_K, DT, VISC, STEP_TOL, MC.ITERS, STEP_MG)
            dens = OB.dens_step(g["dens"], f["dens0"], vel["u"], vel["v"], vel["w"], mask, MC.STEP_K, DT, DIFF)
            outs.append((vel, dens))
            g = dict(f, u=vel["u"], v=vel["v"], w=vel["w"], dens=dens)
        _STEPS[N] = outs
    return _STEPS[N]


@pytest.mark.parametrize("N,P", [(16, 1), (34, 1), (40, 1), (40, 2), (64, 1)], ids=lambda x: str(x))
def test_steps_under_a_mask(N, P):
    dtype = np.float32
    f = random_fields(N, dtype, 91)
    mask = MC.mask("odd_box", N, dtype)
    outs = step_reference(N, f, mask)
    with make(N, dtype, K=MC.STEP_K, P=P) as fs:
        fs.set_pressure_solver("cg", STEP_TOL, MC.ITERS)
        fs.set_pressure_sync(MC.CHECK_EVERY if P > 1 else 0)
        masked_multigrid(fs, mask, STEP_MG, slot="u0")
        upload_all(fs, f)
        for step, (vel, dens) in enumerate(outs):
            fs.vel_step()
            info = fs.pressure_info()
            print(f"P={P} step {step}: {info}")
            assert (info["status"], info["iterations"]) == (vel["status"], vel["iterations"])
            assert vel["iterations"] >= 1
            fs.dens_step()
            fs.sync()
            for n in ("u", "v", "w"):
                assert_same_bits(fs.download(n), vel[n], f"P={P} step {step}: {n}")
            assert_same_bits(fs.download("dens"), dens, f"P={P} step {step}: dens")
            for n in ("u0", "v0", "w0", "dens0"):
                fs.upload(n, f[n])


# ---- (c) -----------------------------------------------------------------------------------------------------------
DECOMPOSED = [(N, P, L, tr, f) for N, P, L in MC.DECOMPOSED for tr in ("copy", "rccl-self")
              for f in MC.DECOMPOSED_FAMILIES]


@pytest.mark.parametrize("N,P,L,transport,family", DECOMPOSED,
                         ids=[f"{f}-N{n}-P{p}-L{l}-{tr}" for n, p, l, tr, f in DECOMPOSED])
def test_every_decomposition(N, P, L, transport, family):
    """The P = 1 references: the cycle alone and four iterations, the scalars on the device for the rccl-self runs."""
    dtype = np.float32 if transport == "copy" else np.float64
    s = (2, L, 8)
    mask = MC.mask(family, N, dtype, P)
    with make(N, dtype, P=P, transport=transport) as fs:
        masked_multigrid(fs, mask, s)
        check_cycle(fs, family, N, dtype, want_cycle(family, N, dtype, s, P), f"{family} N={N} P={P} {transport}", parked=False)
        fs.set_pressure_sync(MC.CHECK_EVERY if transport == "rccl-self" else 0)
        check_solve(fs, family, N, dtype, MC.DECOMPOSED_ITERS, want_solve(family, N, dtype, MC.DECOMPOSED_ITERS, s, P),
                    f"{family} N={N} P={P} {transport}")
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


# ---- (d) -----------------------------------------------------------------------------------------------------------
def test_the_setting_off_still_refuses():
    N, dtype = 16, np.float32
    invalid = S().SF_ERR_INVALID
    with make(N, dtype) as fs:
        assert fs.obstacle_multigrid() is False
        assert S().lib.sf_set_obstacle_multigrid(fs._h, 2) == invalid
        upload_all(fs, random_fields(N, dtype, 92))
        fs.set_pressure_solver("cg", 1e-2, 5)
        for ready in (lambda: None, lambda: fs.set_obstacles(MC.mask("box", N, dtype), slot=MASK_SLOT),
                      lambda: fs.set_obstacle_multigrid(True)):
            ready()  # nothing; obstacles without the V-cycle; the setting without the V-cycle
            with pytest.raises(S().SfError) as e:
                fs.precondition_masked("u0", "v0")
            assert e.value.status == invalid
        fs.set_obstacle_multigrid(False)
        fs.set_pressure_multigrid(2)
        for call in (fs.vel_step, lambda: fs.project_cg("u", "v", "w", "u0", "v0", 1e-2, 5),
                     lambda: fs.precondition_masked("u0", "v0")):
            with pytest.raises(S().SfError) as e:
                call()
            assert e.value.status == invalid and ("multigrid" in str(e.value))
        fs.set_obstacle_multigrid(True)
        with pytest.raises(S().SfError) as e:
            fs.precondition_masked("u0", "u0")
        assert e.value.status == invalid
        fs.vel_step()
        assert fs.pressure_info()["iterations"] >= 1


def test_switching_obstacles_off_is_the_unmasked_cycle():
    """The setting on, a masked cycle, then set_obstacles(None): sf_precondition and the solve are §11.3's, bit for bit
    and launch for launch."""
    N, dtype, family = 16, np.float32, "odd_box"
    path = os.environ["SF_TRACE_SCHEDULE"]
    z0, r = MC.rhs_fields(family, N, dtype)
    with make(N, dtype) as fs:
        masked_multigrid(fs, MC.mask(family, N, dtype), MC.DEFAULT)
        check_cycle(fs, family, N, dtype, want_cycle(family, N, dtype, MC.DEFAULT), "masked", parked=False)
        names = {op["name"] for op in slab0_ops(path)}
        assert {"mg_coarsen_mask", "mg_face_code", "mg_smooth0_masked", "mg_smooth_masked", "mg_restrict_masked",
                "mg_prolong_masked"} <= names and not names & {"mg_smooth0", "mg_smooth", "mg_restrict", "mg_prolong"}
        fs.set_obstacles(None)
        start = len(slab0_ops(path))
        fs.upload("u0", z0)
        fs.precondition("u0", "v0")
        fs.sync()
        assert_same_bits(fs.download("u0"), G.vcycle(r[I, I, I], *MC.DEFAULT), "unmasked again")
        vel = MC.velocity(family, N, dtype)
        for n, a in zip(("u", "v", "w"), vel):
            fs.upload(n, a)
        info = fs.project_cg("u", "v", "w", "u0", "v0", MC.TOL, 3)
        want = G.project_cg(*vel, MC.TOL, 3, *MC.DEFAULT)
        assert (info["status"], info["iterations"]) == (want["status"], want["iterations"])
        for slot, name in OUT:
            assert_same_bits(fs.download(slot), want[name], name)
        after = [op["name"] for op in slab0_ops(path)[start:]]
        assert "mg_smooth" in after and not any("masked" in n or n in ("mg_coarsen_mask", "mg_face_code") for n in after)


def test_an_empty_mask_is_the_unmasked_cycle():
    N, dtype = 34, np.float64
    _, r = MC.rhs_fields("empty", N, dtype)
    with make(N, dtype) as fs:
        masked_multigrid(fs, MC.mask("empty", N, dtype), MC.DEFAULT)
        check_cycle(fs, "empty", N, dtype, G.vcycle(r[I, I, I], *MC.DEFAULT), "empty mask against pressure_mg_ref")


def test_a_second_mask_and_another_depth_are_honoured():
    """The level codes follow a second sf_set_obstacles and a sf_set_pressure_multigrid with another max_levels, in
    either order with the setting itself."""
    N, dtype, first, second = MC.SECOND_MASK
    with make(N, dtype) as fs:
        fs.set_obstacle_multigrid(True)  # (before the two it goes with)
        fs.set_pressure_multigrid(*MC.DEFAULT)
        fs.set_obstacles(MC.mask(first, N, dtype), slot=MASK_SLOT)
        check_cycle(fs, first, N, dtype, want_cycle(first, N, dtype, MC.DEFAULT), "first mask", parked=False)
        fs.set_obstacles(MC.mask(second, N, dtype), slot=MASK_SLOT)
        check_cycle(fs, second, N, dtype, want_cycle(second, N, dtype, MC.DEFAULT), "second mask", parked=False)
        for s in ((2, 2, 8), MC.SHORT, MC.DEFAULT):
            fs.set_pressure_multigrid(*s)
            check_cycle(fs, second, N, dtype, want_cycle(second, N, dtype, s), f"second mask, {s}", parked=False)
        fs.set_obstacles(MC.mask(first, N, dtype), slot=MASK_SLOT)
        check_solve(fs, first, N, dtype, MC.ITERS, want_solve(first, N, dtype, MC.ITERS, MC.DEFAULT), "first mask again")
