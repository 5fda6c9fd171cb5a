"""The masked kernels of docs/SPEC.md §15 to §17 on special values that are operands, and the three-field forms of the
masked sweep and advect at every row shape; the inputs and case tables are tests/obstacle_special_cases.py, everything
is held to the bits of the numpy references.

(i)   sf_diffuse_masked and sf_advect_masked (one field) on four families of inputs - NaN, +-inf and zeros of either sign
      in fluid cells next to solids; zeros whose sign the mask decides; subnormals; back-traces that land exactly on a
      cell centre with a zero weight on a solid sample - at N = 5, 13, 34, 65, 70, both precisions, b = 0 .. 3, K = 1, 2,
      4; the sweep at a second-trip size per precision; one case over two slabs, over both transports.
(ii)  sf_project_cg under a mask on all-zero, zero-region and subnormal velocities, none and jacobi:2, scalars on the host
      and on the device; sf_precondition_masked on an all-zero and on a subnormal right-hand side.
(iii) vel_step + dens_step with sf_set_obstacle_transport(1), which alone reach lin_solve_masked_kernel<T, 3> and
      advect_masked_kernel<T, 3>: against the step composed in numpy at N = 1 .. 70, and at the second-trip sizes
      against the same step composed from the public single-field operators on a second context.
tests/test_obstacle_special_inputs_ref.py shows on the CPU which wrong readings of the kernels' arithmetic these cases
tell from the right one, and that the conditions each case relies on hold. The schedule-hazard check of
tests/conftest.py reads the trace of every context created here."""
import numpy as np
import pytest

import diagnostics_ref as D
import obstacle_cases as OC
import obstacle_mg_cases as MC
import obstacle_special_cases as SP
import obstacle_transport_cases as TC
import obstacles_ref as OB
import shape_cases as C
from gpu_support import DIFF, VISC, assert_same_bits, make, upload_all
from shape_cases import dname

pytestmark = pytest.mark.gpu

MASK_SLOT = "v0"   # a slot no single operator below touches
SOLVE_SLOT = "dens0"  # a slot neither the projection nor sf_precondition_masked touches
I = SP.I


def transport_on(fs, mask, slot=MASK_SLOT):
    fs.set_obstacles(mask, slot=slot)
    fs.fill(slot, float("nan"))  # the mask is read once
    fs.set_obstacle_transport(True)
    assert fs.obstacle_transport() is True


def nan_planted(*fields):
    return any(np.isnan(f).any() for f in fields)


def check_sweep(fs, b, K, x, x0, want, what):
    """nan_ok where the inputs hold a NaN: its payload is the hardware's to choose."""
    fs.set_iters(K)
    fs.upload("dens", x)
    fs.upload("u0", x0)
    fs.diffuse_masked(b, "dens", "u0", TC.DIFF)
    fs.sync()
    assert_same_bits(fs.download("dens"), want, f"{what}: diffuse_masked b={b} K={K}", nan_ok=np.isnan(want).any())
    assert_same_bits(fs.download("u0"), x0, f"{what}: x0 is left alone", nan_ok=nan_planted(x0))


def check_advect(fs, b, d0, vel, want, what):
    for n, a in zip(("u", "v", "w"), vel):
        fs.upload(n, a)
    fs.upload("u0", d0)
    fs.fill("dens", float("nan"))  # every entry of the result is written
    fs.advect_masked(b, "dens", "u0", "u", "v", "w")
    fs.sync()
    assert_same_bits(fs.download("dens"), want, f"{what}: advect_masked b={b}", nan_ok=np.isnan(want).any())


# ---- (i) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,mfam,N,dtype", SP.OPERATORS, ids=[SP.operator_id(*c) for c in SP.OPERATORS])
def test_single_operators_on_special_inputs(family, mfam, N, dtype):
    """Non-finite velocities (specials from N = 13 on) on one slab: the clamps, the NaN guard and the integer clamp of the
    back-trace keep every sample address inside the stored planes."""
    mask = OC.mask(mfam, N, dtype)
    want = SP.operator_case(family, mfam, N, dtype)
    what = SP.operator_id(family, mfam, N, dtype)
    with make(N, dtype) as fs:
        transport_on(fs, mask)
        for b in TC.BS:
            K = SP.sweeps(N, b)
            x, x0, _ = SP.sweep_inputs(family, mask, b, K)
            check_sweep(fs, b, K, x, x0, want["sweep", b, K], what)
            d0, u, v, w, _ = SP.advect_inputs(family, mfam, mask, b)
            check_advect(fs, b, d0, (u, v, w), want["advect", b], what)


@pytest.mark.parametrize("N,dtype", SP.LANDING, ids=[SP.landing_id(*c) for c in SP.LANDING])
def test_exact_landings_under_a_mask(N, dtype):
    """dt = 0.125: every trace lands on a cell centre or on a bound; three fluid cells hold +inf, -inf and -0 and take
    a solid sample with weight zero, which multiplies the cell's own value."""
    mask, d0, u, v, w, cells = SP.landing_inputs(N, dtype)
    want = SP.landing_case(N, dtype)["advect", 0]
    with make(N, dtype) as fs:
        fs.set_coefficients(C.LANDING_DT, DIFF, VISC)
        transport_on(fs, mask)
        check_advect(fs, 0, d0, (u, v, w), want, SP.landing_id(N, dtype))
        got = fs.download("dens")[I]
        assert np.isnan(got[cells[0]]) and np.isnan(got[cells[1]])


@pytest.mark.parametrize("N,dtype", SP.SECOND_TRIP, ids=[f"N{n}-{dname(t)}" for n, t in SP.SECOND_TRIP])
def test_the_sweep_at_a_second_trip(N, dtype):
    """walls, K = 1: every special value on cells 64 W and 64 W + 1 of a row, the seam of the row kernels' lane loop."""
    mask = OC.mask("walls", N, dtype)
    (_, b, K), want = next(iter(SP.second_trip_case(N, dtype).items()))
    x, x0, _ = SP.sweep_inputs("specials", mask, b, K)
    with make(N, dtype) as fs:
        transport_on(fs, mask)
        check_sweep(fs, b, K, x, x0, want, f"second trip N={N}")


@pytest.mark.parametrize("N,P,transport,dtype", SP.DECOMPOSED, ids=[f"N{n}-P{p}-{tr}" for n, p, tr, _ in SP.DECOMPOSED])
def test_specials_on_both_sides_of_a_slab_boundary(N, P, transport, dtype):
    """The P = 1 reference; finite velocities of less than one plane (a NaN w on a decomposed context is a reported halo
    violation, SPEC §4), every special value in the fields on the last plane of slab 0 and on the first of slab 1."""
    mask, lin, adv, vel = SP.decomposed_inputs(N, P, dtype)
    want = SP.decomposed_case(N, P, dtype)
    what = f"N={N} P={P} {transport}"
    with make(N, dtype, P=P, transport=transport) as fs:
        transport_on(fs, mask)
        for b in TC.BS:
            x, x0, K = lin[b]
            check_sweep(fs, b, K, x, x0, want["sweep", b, K], what)
            check_advect(fs, b, adv[b], vel, want["advect", b], what)
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


# ---- (ii) ----------------------------------------------------------------------------------------------------------
OUT = (("u", "u"), ("v", "v"), ("w", "w"), ("u0", "p"), ("v0", "div"))
PROJECT = [(k, *c) for k in SP.PROJECT_KINDS for c in SP.PROJECTIONS]


@pytest.mark.parametrize("kind,N,dtype,mfam", PROJECT, ids=[SP.project_id(k, n, t, m) for k, n, t, m in PROJECT])
def test_projection_of_special_velocities(kind, N, dtype, mfam):
    """Two iterations at most. An all-zero divergence is CONVERGED with no iteration, an underflowing rho0 whatever the
    reference makes of it: device and reference agree on status, iterations and the bits of rel_residual."""
    mask = OC.mask(mfam, N, dtype)
    vel = SP.project_velocity(kind, mask)
    with make(N, dtype) as fs:
        fs.set_obstacles(mask, slot=SOLVE_SLOT)
        fs.fill(SOLVE_SLOT, float("nan"))
        for m in (0, SP.PROJECT_SWEEPS):
            want = SP.project_case(kind, N, dtype, mfam, m)
            fs.set_pressure_preconditioner("jacobi" if m else "none", m)
            for every in (0, SP.CHECK_EVERY):
                fs.set_pressure_sync(every)
                what = f"{SP.project_id(kind, N, dtype, mfam)} m={m} sync={every}"
                for n, a in zip(("u", "v", "w"), vel):
                    fs.upload(n, a)
                info = fs.project_cg("u", "v", "w", "u0", "v0", OC.TOL, SP.PROJECT_ITERS)
                fs.sync()
                print(f"{what}: got {info} want status {want['status']} iterations {want['iterations']} "
                      f"rel {want['rel_residual']!r}")
                assert (info["status"], info["iterations"]) == (want["status"], want["iterations"]), what
                assert D.bits(info["rel_residual"]) == D.bits(want["rel_residual"]), what
                for slot, name in OUT:
                    assert_same_bits(fs.download(slot), want[name], f"{what}: {name}")


CYCLE = [(k, *c) for k in SP.CYCLE_KINDS for c in SP.CYCLES]


@pytest.mark.parametrize("kind,N,dtype,s,mfam", CYCLE, ids=[SP.cycle_id(k, n, t, s, m) for k, n, t, s, m in CYCLE])
def test_precondition_masked_on_special_right_hand_sides(kind, N, dtype, s, mfam):
    mask = MC.mask(mfam, N, dtype)
    r = SP.cycle_rhs(kind, mask)
    want = SP.cycle_case(kind, N, dtype, s, mfam)
    with make(N, dtype) as fs:
        fs.set_obstacles(mask, slot=SOLVE_SLOT)
        fs.fill(SOLVE_SLOT, float("nan"))
        fs.set_pressure_multigrid(*s)
        fs.set_obstacle_multigrid(True)
        fs.fill("u0", float("nan"))  # what z held is nothing to z = V_m(0, r)
        fs.upload("v0", r)
        fs.precondition_masked("u0", "v0")
        fs.sync()
        assert_same_bits(fs.download("u0"), want, f"{SP.cycle_id(kind, N, dtype, s, mfam)}: z")
        assert_same_bits(fs.download("v0"), r, "r is left alone")


# ---- (iii) ---------------------------------------------------------------------------------------------------------
def stepping(N, dtype, mask, K, iters):
    """A context with the settings of the step cases: the mask goes through a slot that is scratch before the step."""
    fs = make(N, dtype, K=K)
    fs.set_pressure_solver("cg", SP.STEP_TOL, iters)
    fs.set_pressure_preconditioner("none", 0)
    transport_on(fs, mask, slot="u0")
    return fs


@pytest.mark.parametrize("N,dtype", SP.STEPS, ids=[SP.step_id(*c) for c in SP.STEPS])
def test_a_step_at_every_shape(N, dtype):
    """vel_step + dens_step against obstacle_transport_ref.vel_step / dens_step: random30 at odd N, walls at even N."""
    f = SP.step_fields(N, dtype)
    vel, dens = SP.step_case(N, dtype)
    what = SP.step_id(N, dtype)
    with stepping(N, dtype, SP.step_mask(N, dtype), SP.STEP_K, SP.STEP_ITERS) as fs:
        upload_all(fs, f)
        fs.vel_step()
        info = fs.pressure_info()
        print(f"{what}: {info}")
        assert (info["status"], info["iterations"]) == (vel["status"], vel["iterations"])
        fs.dens_step()
        fs.sync()
        for n in ("u", "v", "w"):
            assert_same_bits(fs.download(n), vel[n], f"{what}: {n}")
        assert_same_bits(fs.download("dens"), dens, f"{what}: dens")


def composed_step(fs):
    """vel_step_body and dens_step_body of the solver spelled with the public single-field operators; a swap of two slots
    there is the other slot's name here."""
    for x, s in (("u", "u0"), ("v", "v0"), ("w", "w0")):
        fs.add_source(x, s)
    for b, x, x0 in ((1, "u0", "u"), (2, "v0", "v"), (3, "w0", "w")):  # (swapped: the sum is the right-hand side)
        fs.diffuse_masked(b, x, x0, VISC)
    fs.project_cg("u0", "v0", "w0", "u", "v", SP.STEP_TOL, 1)
    for b, d, d0 in ((1, "u", "u0"), (2, "v", "v0"), (3, "w", "w0")):  # (swapped back: d0 is the trace velocity too)
        fs.advect_masked(b, d, d0, "u0", "v0", "w0")
    info = fs.project_cg("u", "v", "w", "u0", "v0", SP.STEP_TOL, 1)
    fs.add_source("dens", "dens0")
    fs.diffuse_masked(0, "dens0", "dens", DIFF)
    fs.advect_masked(0, "dens", "dens0", "u", "v", "w")
    return info


@pytest.mark.parametrize("N,dtype,mfam", SP.BIG_STEPS, ids=[f"N{n}-{dname(t)}-{m}" for n, t, m in SP.BIG_STEPS])
def test_a_step_at_the_second_trip_is_its_single_operators(N, dtype, mfam):
    """An identity between two forms of the device code, not a comparison with numpy (a numpy step at 257^3 costs most of a
    minute): vel_step + dens_step, whose masked sweep and advect are the three-field kernels, against the same step
    composed from sf_add_source, sf_diffuse_masked, sf_project_cg and sf_advect_masked, whose kernels are the one-field
    forms, on a second context with the same inputs; K = 1, one CG iteration. The one-field side is anchored to numpy at
    these row shapes by test_the_sweep_at_a_second_trip above and by test_row_shapes_of_the_sweep of
    tests/test_obstacle_transport_gpu.py (the sweep), by test_single_operators_on_special_inputs at N = 65 and 70 (the
    flat advect, whose cell-to-lane map knows no row trip) and by test_one_application_reads_every_shell_as_stored of
    tests/test_obstacles_gpu.py (the projection); the three-field side by test_a_step_at_every_shape up to N = 70."""
    f = SP.big_step_fields(N, dtype, 300 + N)
    mask = OC.mask(mfam, N, dtype)
    with stepping(N, dtype, mask, 1, 1) as fs:
        upload_all(fs, f)
        fs.vel_step()
        stepped = fs.pressure_info()
        fs.dens_step()
        fs.sync()
        want = {n: fs.download(n) for n in ("u", "v", "w", "dens")}
    with stepping(N, dtype, mask, 1, 1) as fs:
        upload_all(fs, f)
        info = composed_step(fs)
        fs.sync()
        assert (info["status"], info["iterations"]) == (stepped["status"], stepped["iterations"])
        assert info["iterations"] == 1
        for n, a in want.items():
            assert np.isfinite(a).all() and a[I].any()
            assert_same_bits(fs.download(n), a, f"N={N} {dname(dtype)} {mfam}: {n}")
    solid = OB.Mask(mask).solid
    assert not want["dens"][I][solid].any() and want["dens"][I][~solid].any()
