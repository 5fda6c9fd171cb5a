"""Moving solids on the device (docs/SPEC.md §19, sf_set_obstacle_velocity): everything is held to the bits of
tests/obstacle_moving_ref.py on the masks of tests/obstacle_cases.py and the inputs of tests/obstacle_moving_cases.py.

(a) sf_project_cg (plain CG, jacobi:2 and the masked V-cycle), sf_diffuse_masked (K = 1, 2, 5) and
    sf_advect_masked (b = 0 .. 3) under every mask family at every size class, both precisions, with three independent
    random solid-velocity fields, and once more with a NaN parked in every fluid and shell entry of them;
(b) the three row kernels where a row takes a second trip of the lane loop, with closed faces and solid cells planted
    on both sides of the lane seam and on the last cell of a row;
(c) four decompositions over each of the two transports, walls (solids on both sides of every slab boundary);
(d) vel_step + dens_step against the step composed in numpy: the three solvers, bound and unbound sources, forces, one
    slab and each of the four decompositions, and one step at every size so that the three-field forms run at every row
    shape; at the second-trip sizes 131 (fp64), 257 and 262 (fp32), where a numpy step costs most of a minute, the step
    against the same step composed on the device from the one-field operators, which (b) holds to numpy there;
(e) a box moved one cell between two steps, mask and velocity set again;
(f) a zero velocity gives the bits of the same context with the velocity unset;
(g) switching the velocity off, or never setting it, leaves the launches of the parent;
(h) the refusals (sf_advect_maccormack_masked of a velocity component among them), the getter, the slots being free again, SF_GRAPH=1 around the setter.
tests/test_obstacle_moving_ref.py shows on the CPU which wrong readings of §19 these cases tell from the right one.
The schedule-hazard check of tests/conftest.py reads the trace of every context created here."""
import os
import time

import numpy as np
import pytest

import obstacle_cases as OC
import obstacle_moving_cases as MV
import obstacle_maccormack_ref as OMC
import obstacle_moving_ref as MR
import obstacle_transport_cases as TC
import obstacle_transport_ref as TR
import obstacles_ref as OB
import shape_cases as C
from gpu_support import (DIFF, DT, USER, VISC, S, assert_same_bits, make, random_fields, set_forces, slab0_ops,
                         upload_all)

pytestmark = pytest.mark.gpu

MASK_SLOT = "w0"  # a slot no single operator below touches
VS_SLOTS = ("user0", "user1", "user2")
_WANT = {}
NAN = float("nan")


def once(key, build):
    """A reference computed once per case and only read afterwards."""
    if key not in _WANT:
        t0 = time.perf_counter()
        _WANT[key] = build()
        if time.perf_counter() - t0 > 0.5:
            print(f"reference {key}: {time.perf_counter() - t0:.1f} s")
    return _WANT[key]


def set_velocity(fs, vs):
    """The solid velocity through the three user slots, which are overwritten afterwards: it is read once."""
    fs.set_obstacle_velocity(*vs, slots=VS_SLOTS)
    for slot in VS_SLOTS:
        fs.fill(slot, NAN)
    assert fs.obstacle_velocity() is True


def moving_on(fs, mask, vs, slot=MASK_SLOT, order=0):
    """Obstacles, the transport setting and the solid velocity, in one of three orders."""
    assert fs.obstacle_velocity() is False
    steps = [lambda: fs.set_obstacle_transport(True), lambda: (fs.set_obstacles(mask, slot=slot), fs.fill(slot, NAN)),
             lambda: set_velocity(fs, vs)]
    for k in range(3):
        steps[(k + order) % 3]()


def set_solver(fs, solver, tol=MV.TOL, iters=MV.ITERS):
    name, m, mg = solver
    fs.set_pressure_solver("cg", tol, iters)
    if mg:
        fs.set_pressure_multigrid(*mg)
        fs.set_obstacle_multigrid(True)
    else:
        fs.set_pressure_multigrid(0)
        fs.set_pressure_preconditioner("jacobi" if m else "none", m)


def check_project(fs, fields, want, what, tol=MV.TOL, iters=MV.ITERS):
    for n, a in zip(("u", "v", "w"), fields):
        fs.upload(n, a)
    fs.fill("u0", NAN)
    fs.fill("v0", NAN)
    info = fs.project_cg("u", "v", "w", "u0", "v0", tol, iters)
    fs.sync()
    print(f"{what}: got {info} want {want['status']} {want['iterations']} {want['rel_residual']!r}")
    assert (info["status"], info["iterations"]) == (want["status"], want["iterations"]), what
    assert np.float64(info["rel_residual"]).tobytes() == np.float64(want["rel_residual"]).tobytes(), what
    for slot, name in (("u", "u"), ("v", "v"), ("w", "w"), ("u0", "p"), ("v0", "div")):
        assert_same_bits(fs.download(slot), want[name], f"{what}: {name}")


def check_diffuse(fs, fields, b, K, want, what):
    x, x0 = fields
    fs.set_iters(K)
    fs.upload("dens", x)
    fs.upload("u0", x0)
    fs.diffuse_masked(b, "dens", "u0", MV.DIFF)
    fs.sync()
    assert_same_bits(fs.download("dens"), want, f"{what}: diffuse_masked b={b} K={K}")


def check_advect(fs, d0, b, want, what):
    fs.upload("u0", d0)
    fs.fill("dens", NAN)  # every entry of the result is written
    fs.advect_masked(b, "dens", "u0", "u", "v", "w")
    fs.sync()
    assert_same_bits(fs.download("dens"), want, f"{what}: advect_masked b={b}")


def transport_vs(family, N, dtype):
    return MV.solid_velocity(family, N, dtype, MV.transport_scale(N))


def want_project(family, N, dtype, solver, P=None):
    name, m, mg = solver
    return once(("project", family, N, C.dname(dtype), name, P), lambda: MR.project_cg(
        *MV.project_fields(family, N, dtype), OC.mask(family, N, dtype, P), MV.solid_velocity(family, N, dtype), MV.TOL,
        MV.ITERS, m, mg))


def want_diffuse(family, N, dtype, b, K, P=None):
    def build():
        x, x0 = TC.fields(family, N, dtype, b)
        MR.diffuse(b, x, x0, MV.DIFF, DT, K, OC.mask(family, N, dtype, P), transport_vs(family, N, dtype))
        return x
    return once(("diffuse", family, N, C.dname(dtype), b, K, P), build)


def want_advect(family, N, dtype, b, one_plane=False, P=None):
    def build():
        d0 = TC.fields(family, N, dtype, b)[1]
        d = np.zeros_like(d0)
        MR.advect(b, d, d0, *TC.velocity(family, N, dtype, one_plane), DT, OC.mask(family, N, dtype, P),
                  transport_vs(family, N, dtype))
        return d
    return once(("advect", family, N, C.dname(dtype), b, one_plane, P), build)


# ---- (a) -----------------------------------------------------------------------------------------------------------
OPERATORS = [(f, N, t) for f in MV.FAMILIES for N in MV.SIZES for t in C.DTYPES]


@pytest.mark.parametrize("family,N,dtype", OPERATORS, ids=[f"{f}-N{n}-{C.dname(t)}" for f, n, t in OPERATORS])
def test_single_operators_under_every_family(family, N, dtype):
    mask = OC.mask(family, N, dtype)
    what = f"{family} N={N} {C.dname(dtype)}"
    pv, tv = MV.solid_velocity(family, N, dtype), transport_vs(family, N, dtype)
    solvers = MV.SOLVERS
    with make(N, dtype) as fs:
        moving_on(fs, mask, pv, order=N % 3)
        for parked in (False, True):
            tag = what + (" parked NaN" if parked else "")
            set_velocity(fs, MV.parked(pv, mask) if parked else pv)
            for solver in solvers[:1] if parked else solvers:
                set_solver(fs, solver)
                check_project(fs, MV.project_fields(family, N, dtype), want_project(family, N, dtype, solver), f"{tag} {solver[0]}")
            set_velocity(fs, MV.parked(tv, mask) if parked else tv)
            for n, a in zip(("u", "v", "w"), TC.velocity(family, N, dtype)):
                fs.upload(n, a)
            for b in MV.BS:
                for K in (2,) if parked else MV.SWEEPS:
                    check_diffuse(fs, TC.fields(family, N, dtype, b), b, K, want_diffuse(family, N, dtype, b, K), tag)
                check_advect(fs, TC.fields(family, N, dtype, b)[1], b, want_advect(family, N, dtype, b), tag)
                got = fs.download("dens")
                assert np.isfinite(got).all(), tag


# ---- (b) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", MV.ROW_SHAPES, ids=[f"N{n}-{C.dname(t)}" for n, t in MV.ROW_SHAPES])
def test_the_second_trip_of_a_row(N, dtype):
    """One sweep (b by size) against the reference; the projection against the whole reference in fp64 and, in fp32
    (18 million cells), its two row kernels against the reference's divergence and against the reference's gradient
    subtraction of the pressure the device itself found: one iteration, the CG loop being the merged one."""
    mask = MV.row_mask(N, dtype)
    u, v, w, us, vs, ws, x, x0 = MV.row_fields(N, dtype, 8)
    sv = [us, vs, ws]
    b = N % 3 + 1
    what = f"row N={N} {C.dname(dtype)}"
    with make(N, dtype) as fs:
        moving_on(fs, mask, sv)
        want = x.copy()
        MR.diffuse(b, want, x0, MV.DIFF, DT, 1, mask, sv)
        check_diffuse(fs, (x, x0), b, 1, want, what)
        set_solver(fs, MV.SOLVERS[0])
        if dtype == np.float64:
            check_project(fs, (u, v, w), MR.project_cg(u, v, w, mask, sv, MV.TOL, 1), what, iters=1)
            return
        for n, a in zip(("u", "v", "w"), (u, v, w)):
            fs.upload(n, a)
        fs.project_cg("u", "v", "w", "u0", "v0", MV.TOL, 1)
        fs.sync()
        mk = MR.Moving(mask, sv)
        assert_same_bits(fs.download("v0"), MR.divergence(u, v, w, mk)[1], f"{what}: div")
        p = fs.download("u0")
        MR.subtract_gradient(u, v, w, p, mk)
        for n, a in zip(("u", "v", "w"), (u, v, w)):
            assert_same_bits(fs.download(n), a, f"{what}: {n}")


# ---- (c) -----------------------------------------------------------------------------------------------------------
DECOMPOSED = [(N, P, tr) for N, P in MV.DECOMPOSED for tr in ("copy", "rccl-self")]


@pytest.mark.parametrize("N,P,transport", DECOMPOSED, ids=[f"walls-N{n}-P{p}-{tr}" for n, p, tr in DECOMPOSED])
def test_every_decomposition(N, P, transport):
    """The P = 1 reference. The walls mask has solid cells on both sides of every boundary of these P slabs, so the k
    faces and the samples of a slab's first and last plane take the solid velocity from its ghost planes."""
    family = "walls"
    dtype = np.float32 if P != 17 else np.float64
    mask = OC.mask(family, N, dtype, P)
    what = f"{family} N={N} P={P} {transport}"
    solver = MV.SOLVERS[1]
    with make(N, dtype, P=P, transport=transport) as fs:
        moving_on(fs, mask, MV.solid_velocity(family, N, dtype), order=P % 3)
        set_solver(fs, solver)
        check_project(fs, MV.project_fields(family, N, dtype), want_project(family, N, dtype, solver, P), what)
        set_velocity(fs, transport_vs(family, N, dtype))
        for n, a in zip(("u", "v", "w"), TC.velocity(family, N, dtype, one_plane=True)):
            fs.upload(n, a)
        for b in MV.BS:
            check_diffuse(fs, TC.fields(family, N, dtype, b), b, 5, want_diffuse(family, N, dtype, b, 5, P), what)
            check_advect(fs, TC.fields(family, N, dtype, b)[1], b, want_advect(family, N, dtype, b, True, P), what)
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


# ---- (d) -----------------------------------------------------------------------------------------------------------
STEP_TOL, STEP_ITERS, STEP_K = 1e-2, 10, 6
FORCES = dict(eps=0.3, beta=0.5, ambient=0.1, axis=1)
SOLVER = {s[0]: s for s in MV.SOLVERS}
SOLVER["mg1"] = ("mg1", 0, (2, 1, 8))  # the one-level cycle, the depth two slabs of 17 planes admit
# (N, dtype, solver, bound sources, forces, P, check_every, steps, K)
STEPS = ([(13, np.float64, s, bound, bound and s == "cg", 1, 4 if bound else 0, 2, STEP_K) for s in ("cg", "jacobi2", "mg")
          for bound in (False, True)]
         + [(34, np.float32, "cg", True, False, 2, 4, 2, STEP_K), (34, np.float32, "jacobi2", False, True, 2, 0, 2, STEP_K),
            (34, np.float32, "mg1", True, False, 2, 4, 2, STEP_K), (34, np.float64, "mg", False, False, 1, 0, 2, STEP_K)]
         # one short step on each of the other decompositions
         + [(34, np.float64, "jacobi2", False, False, 17, 0, 1, 2), (64, np.float32, "cg", True, False, 4, 4, 1, 2),
            (40, np.float32, "jacobi2", False, True, 2, 0, 1, 2)]
         # one short step at every size: the three-field forms at every row shape
         + [(N, t, "cg", False, False, 1, 0, 1, 2) for N in MV.SIZES for t in C.DTYPES if (N, t) != (13, np.float64)]
         + [(129, np.float64, "cg", False, False, 1, 0, 1, 1)])


def step_inputs(N, dtype):
    f = random_fields(N, dtype, 191)
    family = "box" if N >= 5 else "walls"
    return f, OC.mask(family, N, dtype), MV.solid_velocity(family, N, dtype, 0.05)


def step_reference(N, dtype, solver, bound, forces, steps, K):
    """vel_step + dens_step composed from the references; the x0 slots hold the sources again before each step."""
    def build():
        f, mask, vs = step_inputs(N, dtype)
        _, m, mg = SOLVER[solver]
        project = lambda u, v, w: MR.project_cg(u, v, w, mask, vs, STEP_TOL, STEP_ITERS, m, mg)  # noqa: E731
        g, outs = dict(f), []
        src = {n: f[n] for n in ("u0", "v0", "w0")} if bound else None
        for _ in range(steps):
            vel = MR.vel_step(g, mask, vs, K, DT, VISC, project, sources=src, forces=FORCES if forces else None)
            dens = MR.dens_step(g["dens"], f["dens0"], vel["u"], vel["v"], vel["w"], mask, K, DT, DIFF)
            outs.append((vel, dens))
            g = dict(f, u=vel["u"], v=vel["v"], w=vel["w"], dens=dens)
        return outs
    return once(("steps", N, C.dname(dtype), solver, bound, forces, steps, K), build)


@pytest.mark.parametrize("N,dtype,solver,bound,forces,P,every,steps,K", STEPS,
                         ids=[f"N{n}-{C.dname(t)}-{s}-{'bound' if b else 'unbound'}-{'forces' if f else 'plain'}-P{p}-sync{e}-"
                              f"{st}x-K{k}" for n, t, s, b, f, p, e, st, k in STEPS])
def test_steps(N, dtype, solver, bound, forces, P, every, steps, K):
    f, mask, vs = step_inputs(N, dtype)
    outs = step_reference(N, dtype, solver, bound, forces, steps, K)
    solid = OB.Mask(mask).solid
    what = f"N={N} {C.dname(dtype)} {solver} bound={bound} forces={forces} P={P} sync={every}"
    with make(N, dtype, K=K, P=P, transport="rccl-self" if bound else "copy") as fs:
        set_solver(fs, SOLVER[solver], STEP_TOL, STEP_ITERS)
        fs.set_pressure_sync(every)
        if forces:
            set_forces(fs, **FORCES)
        # (every user slot may be bound: the mask and the solid velocity go through slots that are scratch before the
        # first step)
        fs.set_obstacle_transport(True)
        fs.set_obstacles(mask, slot="u0")
        fs.set_obstacle_velocity(*vs, slots=("u0", "v0", "w0"))
        upload_all(fs, f)
        if bound:
            for n, slot in USER.items():
                fs.upload(slot, f[n])
            fs.bind_sources()
        for step, (vel, dens) in enumerate(outs):
            fs.vel_step()
            info = fs.pressure_info()
            print(f"{what} step {step}: {info}")
            assert (info["status"], info["iterations"]) == (vel["status"], vel["iterations"])
            fs.dens_step()
            fs.sync()
            for n in ("u", "v", "w"):
                assert_same_bits(fs.download(n), vel[n], f"{what} step {step}: {n}")
            assert_same_bits(fs.download("dens"), dens, f"{what} step {step}: dens")
            if solid.any():  # the velocity field shows the solid moving
                assert_same_bits(fs.download("u")[1:-1, 1:-1, 1:-1][solid], vs[0][1:-1, 1:-1, 1:-1][solid], "u in the solid")
            if not bound:
                for n in ("u0", "v0", "w0", "dens0"):
                    fs.upload(n, f[n])


def composed_step(fs, tol, iters):
    """vel_step_body and dens_step_body of the solver spelled with the public single-field operators; a swap of two slots
    there is the other slot's name here."""
    for x, s in (("u", "u0"), ("v", "v0"), ("w", "w0")):
        fs.add_source(x, s)
    for b, x, x0 in ((1, "u0", "u"), (2, "v0", "v"), (3, "w0", "w")):  # (swapped: the sum is the right-hand side)
        fs.diffuse_masked(b, x, x0, VISC)
    fs.project_cg("u0", "v0", "w0", "u", "v", tol, iters)
    for b, d, d0 in ((1, "u", "u0"), (2, "v", "v0"), (3, "w", "w0")):  # (swapped back: d0 is the trace velocity too)
        fs.advect_masked(b, d, d0, "u0", "v0", "w0")
    info = fs.project_cg("u", "v", "w", "u0", "v0", tol, iters)
    fs.add_source("dens", "dens0")
    fs.diffuse_masked(0, "dens0", "dens", DIFF)
    fs.advect_masked(0, "dens", "dens0", "u", "v", "w")
    return info


BIG_STEPS = [(131, np.float64), (257, np.float32), (262, np.float32)]  # K = 1, max_iters = 1


@pytest.mark.parametrize("N,dtype", BIG_STEPS, ids=[f"N{n}-{C.dname(t)}" for n, t in BIG_STEPS])
def test_a_step_at_the_second_trip_is_its_single_operators(N, dtype):
    """An identity between two forms of the device code, not a comparison with numpy: vel_step + dens_step, whose moving
    sweep and advect are the three-field kernels, against the same step composed from sf_add_source, sf_diffuse_masked,
    sf_project_cg and sf_advect_masked, whose kernels are the one-field forms, on a second context with the same
    inputs; K = 1, one CG iteration. The one-field sweep and the two project halves are held to numpy at these sizes by
    test_the_second_trip_of_a_row, the flat advect (whose cell-to-lane map knows no row trip) at N = 65 and 70 by
    test_single_operators_under_every_family, and the three-field side up to N = 129 by test_steps."""
    mask = MV.row_mask(N, dtype)
    fields = MV.row_fields(N, dtype, 11, 0.05)
    f = dict(zip(("u", "v", "w", "u0", "v0", "w0", "dens", "dens0"), fields))
    vs = fields[8:]
    solid = OB.Mask(mask).solid
    got = []
    for composed in (False, True):
        with make(N, dtype, K=1) as fs:
            fs.set_pressure_solver("cg", STEP_TOL, 1)
            fs.set_pressure_preconditioner("none", 0)
            fs.set_obstacle_transport(True)
            fs.set_obstacles(mask, slot="u0")
            fs.set_obstacle_velocity(*vs, slots=("u0", "v0", "w0"))
            upload_all(fs, f)
            if composed:
                info = composed_step(fs, STEP_TOL, 1)
            else:
                fs.vel_step()
                info = fs.pressure_info()
                fs.dens_step()
            fs.sync()
            got.append((info, {n: fs.download(n) for n in ("u", "v", "w", "dens")}))
    (stepped, want), (info, have) = got
    assert (info["status"], info["iterations"]) == (stepped["status"], stepped["iterations"]) and info["iterations"] == 1
    for n, a in want.items():
        assert np.isfinite(a).all() and a[1:-1, 1:-1, 1:-1].any()
        assert_same_bits(have[n], a, f"N={N} {C.dname(dtype)}: {n}")
    assert_same_bits(want["u"][1:-1, 1:-1, 1:-1][solid], vs[0][1:-1, 1:-1, 1:-1][solid], "u in the solid")
    assert not want["dens"][1:-1, 1:-1, 1:-1][solid].any()


# ---- (e) -----------------------------------------------------------------------------------------------------------
def test_a_moved_box():
    """The sequence of tests/test_obstacle_moving_ref.py: the box one cell further along i in the second step."""
    N, dtype = MV.MOVED_N, np.float32
    outs = once("moved box", MV.moved_box_sequence)
    f = random_fields(N, dtype, 190)
    with make(N, dtype, K=MV.MOVED_K) as fs:
        fs.set_pressure_solver("cg", 1e-2, 10)
        fs.set_obstacle_transport(True)
        upload_all(fs, f)
        for step, (mask, vs, vel, dens) in enumerate(outs):
            fs.set_obstacles(mask, slot="u0")
            fs.set_obstacle_velocity(*vs, slots=("u0", "v0", "w0"))
            for n in ("u0", "v0", "w0", "dens0"):
                fs.upload(n, f[n])
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            for n in ("u", "v", "w"):
                assert_same_bits(fs.download(n), vel[n], f"step {step}: {n}")
            assert_same_bits(fs.download("dens"), dens, f"step {step}: dens")


# ---- (f) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype,P", [(34, np.float32, 1), (34, np.float64, 2), (70, np.float32, 1)],
                         ids=["N34-f32-P1", "N34-f64-P2", "N70-f32-P1"])
def test_zero_velocity_is_the_context_without_one(N, dtype, P):
    """An identity between the new and the merged device code: us = vs = ws = +0 against the velocity unset, on inputs
    without a zero (SPEC §19 "Zero velocity")."""
    family = "random30"
    mask = OC.mask(family, N, dtype, P)
    f = random_fields(N, dtype, 192)
    got = []
    for moving in (False, True):
        out = {}
        with make(N, dtype, K=3, P=P) as fs:
            set_solver(fs, MV.SOLVERS[1], STEP_TOL, 6)
            fs.set_obstacle_transport(True)
            fs.set_obstacles(mask, slot=MASK_SLOT)
            if moving:
                set_velocity(fs, MV.zero_velocity(N, dtype))
            for n, a in zip(("u", "v", "w"), TC.velocity(family, N, dtype, one_plane=True)):
                fs.upload(n, a)
            for b in (1, 2, 3):
                x, x0 = TC.fields(family, N, dtype, b)
                fs.upload("dens", x)
                fs.upload("u0", x0)
                fs.diffuse_masked(b, "dens", "u0", MV.DIFF)
                out[f"diffuse {b}"] = fs.download("dens")
                fs.advect_masked(b, "dens", "u0", "u", "v", "w")
                out[f"advect {b}"] = fs.download("dens")
            upload_all(fs, f)
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            out.update({n: fs.download(n) for n in ("u", "v", "w", "dens")})
            out["info"] = fs.pressure_info()
        got.append(out)
    assert got[0].pop("info") == got[1].pop("info")
    for n, a in got[0].items():
        assert_same_bits(got[1][n], a, n)


# ---- (g) -----------------------------------------------------------------------------------------------------------
def renumbered(ops):
    """Op records with their buffers numbered by first appearance in the stretch."""
    ids, out = {}, []
    for op in ops:
        acc = [[a[0], ids.setdefault(a[1], len(ids)), a[2], a[3]] for a in op["acc"]]
        out.append((op["name"], op["stream"], acc))
    return out


@pytest.mark.parametrize("P", [1, 2], ids=["P1", "P2"])
def test_switching_off_restores_the_launches(P):
    """A §17 step of a context that had a solid velocity for a step and switched it off, and of one that never called
    the entry point: the same launches on the same planes, the same bits. With the velocity set the step runs the four
    moving kernels and dens_step none of them."""
    N, dtype = 34, np.float32
    path = os.environ["SF_TRACE_SCHEDULE"]
    f = random_fields(N, dtype, 193)
    mask = OC.mask("box", N, dtype, P)
    stretches, results = [], []
    moving_names = {"project_div_moving", "project_sub_moving", "lin_solve_moving", "advect_moving"}
    for ever_set in (False, True):
        with make(N, dtype, K=4, P=P) as fs:
            fs.set_pressure_solver("cg", 1e-2, 5)
            fs.set_pressure_preconditioner("jacobi", 2)
            fs.set_obstacle_transport(True)
            if ever_set:
                fs.set_obstacles(mask, slot="u0")
                fs.set_obstacle_velocity(*MV.solid_velocity("box", N, dtype, 0.05), slots=("u0", "v0", "w0"))
                upload_all(fs, f)
                fs.sync()
                start = len(slab0_ops(path))
                fs.vel_step()
                fs.sync()
                mid = len(slab0_ops(path))
                fs.dens_step()
                fs.sync()
                ops = slab0_ops(path)
                assert moving_names <= {op["name"] for op in ops[start:mid]}
                assert not any("masked" in op["name"] for op in ops[start:mid] if not op["name"].startswith("cg_"))
                assert not moving_names & {op["name"] for op in ops[mid:]}
                fs.set_obstacle_velocity(None, None, None)
                assert fs.obstacle_velocity() is False
            fs.sync()
            start = len(slab0_ops(path))
            fs.set_obstacles(mask, slot="u0")
            upload_all(fs, f)
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            stretches.append(renumbered(slab0_ops(path)[start:]))
            results.append({n: fs.download(n) for n in ("u", "v", "w", "dens")})
    names = [name for name, _, _ in stretches[1]]
    assert len(names) > 20 and "lin_solve_masked" in names and "advect_masked" in names and "project_sub_masked" in names
    assert not moving_names & set(names)
    assert stretches[0] == stretches[1]
    for n, a in results[0].items():
        assert_same_bits(results[1][n], a, n)


# ---- (h) -----------------------------------------------------------------------------------------------------------
def test_refusals_and_the_getter():
    N, dtype = 13, np.float32
    mask = OC.mask("box", N, dtype)
    Sx = S()
    invalid = Sx.SF_ERR_INVALID
    u0, v0, w0 = (Sx.FIELD_IDS[n] for n in ("user0", "user1", "user2"))
    with make(N, dtype) as fs:
        upload_all(fs, random_fields(N, dtype, 194))
        fs.set_pressure_solver("cg", 1e-2, 5)
        assert fs.obstacle_velocity() is False
        bad = ((-1, v0, w0), (u0, -1, -1), (u0, u0, w0), (u0, v0, v0), (w0, v0, w0), (u0, v0, len(Sx.FIELD_IDS)), (-2, v0, w0),
               (u0, 99, w0))
        for on in (False, True):
            for slots in bad:
                assert Sx.lib.sf_set_obstacle_velocity(fs._h, *slots) == invalid, slots
                assert b"set_obstacle_velocity" in Sx.lib.sf_last_error(fs._h)
                assert fs.obstacle_velocity() is on  # unchanged
            if not on:
                fs.set_obstacles(mask, slot=MASK_SLOT)
                set_velocity(fs, MV.solid_velocity("box", N, dtype, 0.05))
        # a velocity without the transport setting: vel_step is refused, the setting stays
        with pytest.raises(Sx.SfError) as e:
            fs.vel_step()
        assert e.value.status == invalid and "sf_set_obstacle_transport" in str(e.value)
        assert fs.obstacle_velocity() is True and fs.obstacle_transport() is False
        fs.dens_step()  # §15's, as before
        fs.set_obstacle_transport(True)
        fs.vel_step()
        # a MacCormack velocity scheme: refused whatever sf_set_obstacle_maccormack says; a MacCormack density is not
        for mc in (False, True):
            fs.set_obstacle_maccormack(mc)
            fs.set_advection(Sx.SF_ADVECT_MACCORMACK, Sx.SF_ADVECT_SEMI_LAGRANGIAN)
            with pytest.raises(Sx.SfError) as e:
                fs.vel_step()
            assert e.value.status == invalid and "MacCormack" in str(e.value) and "sf_set_obstacle_velocity" in str(e.value)
            assert fs.obstacle_velocity() is True
        fs.set_advection(Sx.SF_ADVECT_SEMI_LAGRANGIAN, Sx.SF_ADVECT_MACCORMACK)
        fs.vel_step()
        fs.dens_step()
        # the MacCormack operator singly: no form for a velocity component under a solid velocity; b = 0 is §18's bits
        for b in (1, 2, 3):
            with pytest.raises(Sx.SfError) as e:
                fs.advect_maccormack_masked(b, "dens", "u0", "u", "v", "w")
            assert e.value.status == invalid and "sf_set_obstacle_velocity" in str(e.value)
        u, v, w = TC.velocity("box", N, dtype)
        d0 = TC.fields("box", N, dtype)[1]
        for n, a in (("u", u), ("v", v), ("w", w), ("u0", d0)):
            fs.upload(n, a)
        fs.advect_maccormack_masked(0, "dens", "u0", "u", "v", "w")
        fs.sync()
        want = np.zeros_like(d0)
        OMC.advect_mc_masked(0, want, d0, u, v, w, DT, mask)
        assert_same_bits(fs.download("dens"), want, "advect_maccormack_masked b = 0 with a velocity set")
        upload_all(fs, random_fields(N, dtype, 194))
        fs.set_obstacle_velocity(None, None, None)
        assert fs.obstacle_velocity() is False
        fs.set_advection(Sx.SF_ADVECT_MACCORMACK, Sx.SF_ADVECT_MACCORMACK)
        fs.vel_step()  # §18, as before
        fs.sync()


def test_the_slots_are_free_again():
    """The three slots overwritten after the call, and the mask's: the results are those of the reference, twice."""
    N, dtype, family = 13, np.float64, "random30"
    mask = OC.mask(family, N, dtype)
    vs = MV.solid_velocity(family, N, dtype)
    want = want_project(family, N, dtype, MV.SOLVERS[0])
    with make(N, dtype) as fs:
        fs.set_obstacles(mask, slot=MASK_SLOT)
        fs.set_obstacle_transport(True)
        for slot, a in zip(VS_SLOTS, vs):
            fs.upload(slot, a)
        fs.set_obstacle_velocity(*VS_SLOTS)  # by name: what the slots hold
        set_solver(fs, MV.SOLVERS[0])
        for garbage in (NAN, 1e30):
            for slot in VS_SLOTS + (MASK_SLOT,):
                fs.fill(slot, garbage)
            check_project(fs, MV.project_fields(family, N, dtype), want, f"slots filled with {garbage}")


@pytest.mark.parametrize("K", [4, 5], ids=["K4", "K5"])
def test_graphs_around_the_setter(monkeypatch, K):
    """dens_step (the step SF_GRAPH captures under obstacles) with the velocity unset, set, set again, unset under
    SF_GRAPH=1, with a diffuse_masked of a velocity component in between: the bits of the run without graphs, and
    dens_step the same whether a velocity is set or not."""
    N, dtype = 34, np.float32
    f = random_fields(N, dtype, 195)
    mask = OC.mask("box", N, dtype)
    vs = MV.solid_velocity("box", N, dtype, 0.05)
    sequence = (False, False, True, True, True, False, True)
    runs = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("SF_GRAPH", graph)
        got = []
        with make(N, dtype, K=K) as fs:
            upload_all(fs, f)
            fs.set_obstacles(mask, slot="u0")
            fs.set_obstacle_transport(True)
            for on in sequence:
                if on != fs.obstacle_velocity():
                    fs.set_obstacle_velocity(*(vs if on else (None,) * 3), slots=("u0", "v0", "w0"))
                fs.upload("dens0", f["dens0"])
                fs.dens_step()
                fs.upload("u0", f["u0"])
                fs.upload("v0", f["v0"])
                fs.diffuse_masked(1, "u0", "v0", MV.DIFF)
                fs.sync()
                got.append((fs.download("dens"), fs.download("u0")))
        runs[graph] = got
    for step, (a, b) in enumerate(zip(runs["0"], runs["1"])):
        assert_same_bits(b[0], a[0], f"dens_step {step} with graphs")
        assert_same_bits(b[1], a[1], f"diffuse {step} with graphs")
    vel = [f[n] for n in ("u", "v", "w")]
    dens = f["dens"]
    for step, on in enumerate(sequence):
        dens = TR.dens_step(dens, f["dens0"], *vel, mask, K, DT, DIFF)
        assert_same_bits(runs["1"][step][0], dens, f"dens_step {step}: §17's")
        x = f["u0"].copy()
        if on:
            MR.diffuse(1, x, f["v0"], MV.DIFF, DT, K, mask, vs)
        else:
            TR.diffuse_masked(1, x, f["v0"], MV.DIFF, DT, K, mask)
        assert_same_bits(runs["1"][step][1], x, f"diffuse {step}")
