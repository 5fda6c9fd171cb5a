"""Solid obstacles on the device (docs/SPEC.md §15, sf_set_obstacles): everything is held to the bits of
tests/obstacles_ref.py on the masks of tests/obstacle_cases.py.

(a) sf_project_cg under every mask family at every size class, both precisions, none and jacobi:2, scalars on the host
    and on the device: u, v, w, p, div, status, iterations, rel_residual;
(b) one application of the masked operator (sf_poisson_residual) on fields whose shell cells are independent random
    numbers, the second-trip sizes included, there with a two-iteration solve;
(c) the box run to convergence at N = 34;
(d) every decomposition of shape_cases.DECOMPOSED over each of the two transports, walls and random30;
(e) two vel_step + dens_step with a box against the step composed in numpy, bound and unbound sources, one slab and four;
    SF_GRAPH=1 around switching obstacles on and off;
(f) sf_set_obstacles(-1) restores the launches of a context that never set any;
(g) the refusals.
tests/test_obstacles_ref.py shows on the CPU which wrong readings of §15 these cases tell from the right one. The
schedule-hazard check of tests/conftest.py reads the trace of every context created here, the rccl-self ones of (d)
included."""
import os
import time

import numpy as np
import pytest

import diagnostics_ref as D
import obstacle_cases as OC
import obstacles_ref as OB
import shape_cases as C
from gpu_support import DIFF, DT, VISC, S, assert_same_bits, make, random_fields, slab0_ops, upload_all

pytestmark = pytest.mark.gpu

OUT = (("u", "u"), ("v", "v"), ("w", "w"), ("u0", "p"), ("v0", "div"))
MASK_SLOT = "dens0"  # a slot no projection touches
_REFERENCES = {}


def velocity(N, dtype, family):
    return C.cg_velocity(N, dtype, OC.seed(family, N) + 5000)


def reference(family, N, dtype, iters, m, P=None, tol=OC.TOL):
    """OB.project_cg of the family's mask and velocity: computed once per case, only read afterwards."""
    key = (family, N, C.dname(dtype), iters, m, P, tol)
    if key not in _REFERENCES:
        t0 = time.perf_counter()
        _REFERENCES[key] = OB.project_cg(*velocity(N, dtype, family), OC.mask(family, N, dtype, P), tol, iters, m)
        print(f"reference {key}: {time.perf_counter() - t0:.1f} s")
    return _REFERENCES[key]


def precondition(fs, m):
    fs.set_pressure_preconditioner("jacobi" if m > 0 else "none", m)


def obstacles_on(fs, mask, slot=MASK_SLOT):
    fs.set_obstacles(mask, slot=slot)
    want = int((~(mask[1:-1, 1:-1, 1:-1] > 0)).sum())
    assert fs.obstacles() == {"enabled": 1, "fluid_cells": want}
    fs.fill(slot, float("nan"))  # the mask is read once: what the slot holds afterwards changes nothing


def check_masked_solve(fs, u, v, w, mask, tol, iters, want, what):
    for n, a in (("u", u), ("v", v), ("w", w)):
        fs.upload(n, a)
    info = fs.project_cg("u", "v", "w", "u0", "v0", tol, iters)
    fs.sync()
    print(f"{what}: got {info} want status {want['status']} iterations {want['iterations']} rel {want['rel_residual']!r}")
    assert info["solver"] == S().SF_PRESSURE_CG
    assert (info["status"], info["iterations"]) == (want["status"], want["iterations"]), what
    assert D.bits(info["rel_residual"]) == D.bits(want["rel_residual"]), what
    for slot, name in OUT:
        assert_same_bits(fs.download(slot), want[name], f"{what}: {name}")
    got = fs.poisson_residual("u0", "v0")
    assert D.bits(got) == D.bits(OB.poisson_residual(want["p"], want["div"], mask)), what


# ---- (a) -----------------------------------------------------------------------------------------------------------
PROJECTION = [(f, N, t) for f in OC.FAMILIES for N, t in OC.SHAPES]


@pytest.mark.parametrize("family,N,dtype", PROJECTION, ids=[f"{f}-N{n}-{C.dname(t)}" for f, n, t in PROJECTION])
def test_projection_under_every_family(family, N, dtype):
    """Eight iterations at most, unpreconditioned and with jacobi:2, on the host path and with check_every = 4. The
    velocity holds a NaN in every solid cell: it must reach nothing."""
    mask = OC.mask(family, N, dtype)
    u, v, w = velocity(N, dtype, family)
    parked = OC.parked_nan((u, v, w), OB.Mask(mask).solid)
    with make(N, dtype) as fs:
        obstacles_on(fs, mask)
        for m in (0, OC.SWEEPS):
            want = reference(family, N, dtype, OC.ITERS, m)
            precondition(fs, m)
            for every in (0, OC.CHECK_EVERY):
                fs.set_pressure_sync(every)
                what = f"{family} N={N} {C.dname(dtype)} m={m} sync={every}"
                check_masked_solve(fs, u, v, w, mask, OC.TOL, OC.ITERS, want, what)
            check_masked_solve(fs, *parked, mask, OC.TOL, OC.ITERS, want, f"{family} N={N} m={m}: NaN in the solids")


# ---- (b) -----------------------------------------------------------------------------------------------------------
# walls (solid cells on both sides of every lane seam) at every size; random30 up to the fp64 second-trip sizes (its
# numpy reference at 260^3 alone takes seconds)
RESIDUAL = ([("walls", N, t) for N, t in OC.RESIDUAL_SHAPES]
            + [("random30", N, t) for N, t in OC.RESIDUAL_SHAPES if N <= 131])


@pytest.mark.parametrize("family,N,dtype", RESIDUAL, ids=[f"{f}-N{n}-{C.dname(t)}" for f, n, t in RESIDUAL])
def test_one_application_reads_every_shell_as_stored(family, N, dtype):
    mask = OC.mask(family, N, dtype)
    p, div = C.stored_shell_pair(N, dtype, C.shell_seed(N))
    solid = OB.Mask(mask).solid
    want = OB.poisson_residual(p, div, mask)
    with make(N, dtype) as fs:
        obstacles_on(fs, mask)
        for fields, what in (((p, div), "stored shells"), (OC.parked_nan((p, div), solid)[:1] + [div], "NaN in solid p")):
            fs.upload("u0", fields[0])
            fs.upload("v0", fields[1])
            got = fs.poisson_residual("u0", "v0")
            print(f"{family} N={N} {C.dname(dtype)} {what}: got {got!r} want {want!r}")
            assert np.isfinite(want) and D.bits(got) == D.bits(want)
        if C.second_trip(N, dtype):  # the second trip of the masked init and apply kernels, in one of their two forms
            fs.set_pressure_sync(OC.CHECK_EVERY if family == "walls" else 0)
            check_masked_solve(fs, *velocity(N, dtype, family), mask, OC.TOL, 2, reference(family, N, dtype, 2, 0),
                               f"{family} N={N}: two iterations")


# ---- (c) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dname)
@pytest.mark.parametrize("m", [0, 8], ids=["none", "jacobi8"])
def test_the_box_to_convergence(m, dtype):
    N = OC.CONVERGENCE_N
    mask = OC.mask("box", N, dtype)
    want = reference("box", N, dtype, 400, m)
    assert want["status"] == OB.CONVERGED and 8 < want["iterations"] < 400
    with make(N, dtype) as fs:
        obstacles_on(fs, mask)
        precondition(fs, m)
        for every in (0, 5):
            fs.set_pressure_sync(every)
            check_masked_solve(fs, *velocity(N, dtype, "box"), mask, OC.TOL, 400, want, f"box N={N} m={m} sync={every}")


# ---- (d) -----------------------------------------------------------------------------------------------------------
DECOMPOSED = [(f, N, t, P, tr) for N, P, _ in C.DECOMPOSED for t in C.DTYPES for f in ("walls", "random30")
              for tr in ("copy", "rccl-self")]


def decomposed_iters(N):
    return 6 if N <= 70 else 3  # (the numpy reference of a case stays at seconds)


@pytest.mark.parametrize("family,N,dtype,P,transport", DECOMPOSED,
                         ids=[f"{f}-N{n}-{C.dname(t)}-P{p}-{tr}" for f, n, t, p, tr in DECOMPOSED])
def test_every_decomposition(family, N, dtype, P, transport):
    """The P = 1 reference with jacobi:2; the walls mask has solid cells on both sides of every boundary of these P
    slabs, so the face codes of a slab's first and last plane come from the mask's ghost planes."""
    iters, m = decomposed_iters(N), OC.SWEEPS
    mask = OC.mask(family, N, dtype, P)
    want = reference(family, N, dtype, iters, m, P)
    with make(N, dtype, P=P, transport=transport) as fs:
        obstacles_on(fs, mask)
        precondition(fs, m)
        for every in (0, OC.CHECK_EVERY):
            fs.set_pressure_sync(every)
            check_masked_solve(fs, *velocity(N, dtype, family), mask, OC.TOL, iters, want,
                               f"{family} N={N} P={P} {transport} sync={every}")
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


# ---- (e) -----------------------------------------------------------------------------------------------------------
STEP_TOL, STEP_ITERS, STEP_M = 1e-2, 10, 2
_STEPS = {}


def step_reference(f, mask, bound):
    """Two vel_step + dens_step composed from the references; the x0 slots hold the sources again before each step."""
    if bound not in _STEPS:
        g, outs = dict(f), []
        src = {n: f[n] for n in ("u0", "v0", "w0")} if bound else None
        for _ in range(2):
            vel = OB.vel_step(g, mask, OC.STEP_K, DT, VISC, STEP_TOL, STEP_ITERS, STEP_M, sources=src)
            dens = OB.dens_step(g["dens"], f["dens0"], vel["u"], vel["v"], vel["w"], mask, OC.STEP_K, DT, DIFF)
            outs.append((vel, dens))
            g = dict(f, u=vel["u"], v=vel["v"], w=vel["w"], dens=dens)
        _STEPS[bound] = outs
    return _STEPS[bound]


USER = {"u0": "user0", "v0": "user1", "w0": "user2", "dens0": "user3"}


@pytest.mark.parametrize("bound", [False, True], ids=["unbound", "bound"])
@pytest.mark.parametrize("P", [1, 4], ids=["P1", "P4"])
def test_steps_with_a_box(P, bound):
    N, dtype = OC.STEP_N, np.float32
    f = random_fields(N, dtype, 77)
    mask = OC.mask("box", N, dtype, P)
    outs = step_reference(f, mask, bound)
    solid = OB.Mask(mask).solid
    with make(N, dtype, K=OC.STEP_K, P=P, transport="rccl-self" if bound else "copy") as fs:
        fs.set_pressure_solver("cg", STEP_TOL, STEP_ITERS)
        fs.set_pressure_sync(OC.CHECK_EVERY if P > 1 else 0)
        precondition(fs, STEP_M)
        obstacles_on(fs, mask, slot="u0")  # (every user slot may be bound: a slot that is scratch before the first step)
        upload_all(fs, f)
        if bound:
            for n, slot in USER.items():
                fs.upload(slot, f[n])
            fs.bind_sources()
        for step, (vel, dens) in enumerate(outs):
            fs.vel_step()
            info = fs.pressure_info()
            print(f"P={P} bound={bound} step {step}: {info}")
            assert (info["status"], info["iterations"]) == (vel["status"], vel["iterations"])
            assert vel["iterations"] >= 1
            fs.dens_step()
            fs.sync()
            for n in ("u", "v", "w"):
                assert_same_bits(fs.download(n), vel[n], f"P={P} bound={bound} step {step}: {n}")
            got = fs.download("dens")
            assert_same_bits(got, dens, f"P={P} bound={bound} step {step}: dens")
            assert not got[1:-1, 1:-1, 1:-1][solid].any() and got[1:-1, 1:-1, 1:-1][~solid].any()
            if not bound:
                for n in ("u0", "v0", "w0", "dens0"):
                    fs.upload(n, f[n])


def test_graphs_around_switching_obstacles(monkeypatch):
    """dens_step without, with and again without obstacles under SF_GRAPH=1: the bits of the run without graphs, so no
    cached graph of one form is replayed for the other."""
    N, dtype = OC.STEP_N, np.float32
    f = random_fields(N, dtype, 78)
    mask = OC.mask("box", N, dtype)
    runs = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("SF_GRAPH", graph)
        got = []
        with make(N, dtype, K=OC.STEP_K) as fs:
            upload_all(fs, f)
            for on in (False, False, True, True, False, True):
                if on != bool(fs.obstacles()["enabled"]):
                    fs.set_obstacles(mask if on else None, slot="u0")
                fs.upload("dens0", f["dens0"])
                fs.dens_step()
                fs.sync()
                got.append(fs.download("dens"))
        runs[graph] = got
    solid = OB.Mask(mask).solid
    for step, (a, b) in enumerate(zip(runs["0"], runs["1"])):
        assert_same_bits(b, a, f"dens_step {step} with graphs")
    for step, on in enumerate((False, False, True, True, False, True)):
        assert bool(runs["0"][step][1:-1, 1:-1, 1:-1][solid].any()) == (not on), step


# ---- (f) -----------------------------------------------------------------------------------------------------------
def renumbered(ops):
    """Op records with their buffers numbered by first appearance in the stretch."""
    ids, out = {}, []
    for op in ops:
        acc = [[a[0], ids.setdefault(a[1], len(ids)), a[2], a[3]] for a in op["acc"]]
        out.append((op["name"], op["stream"], acc))
    return out


@pytest.mark.parametrize("P", [1, 2], ids=["P1", "P2"])
def test_switching_off_restores_the_launches(P):
    N, dtype = 34, np.float32
    path = os.environ["SF_TRACE_SCHEDULE"]
    f = random_fields(N, dtype, 79)
    mask = OC.mask("box", N, dtype, P)
    stretches, results = [], []
    for ever_set in (False, True):
        with make(N, dtype, K=4, P=P) as fs:
            upload_all(fs, f)
            fs.set_pressure_solver("cg", 1e-2, 5)
            precondition(fs, 2)
            fs.set_pressure_sync(2)
            if ever_set:
                fs.set_obstacles(mask, slot="u0")
                fs.project_cg("u", "v", "w", "u0", "v0", 1e-2, 3)
                fs.set_obstacles(None)
                assert fs.obstacles() == {"enabled": 0, "fluid_cells": N ** 3}
                upload_all(fs, f)
            fs.sync()
            start = len(slab0_ops(path))
            fs.vel_step()
            fs.dens_step()
            fs.poisson_residual("u0", "v0")
            fs.sync()
            stretches.append(renumbered(slab0_ops(path)[start:]))
            results.append({n: fs.download(n) for n in ("u", "v", "w", "dens")})
    assert len(stretches[0]) > 20
    assert not any("masked" in name or name in ("face_code", "zero_solid") for name, _, _ in stretches[1])
    assert stretches[0] == stretches[1]
    for n, a in results[0].items():
        assert_same_bits(results[1][n], a, n)


# ---- (g) -----------------------------------------------------------------------------------------------------------
def test_refusals():
    N, dtype = 13, np.float32
    mask = OC.mask("box", N, dtype)
    invalid = S().SF_ERR_INVALID
    with make(N, dtype) as fs:
        assert fs.obstacles() == {"enabled": 0, "fluid_cells": N ** 3}
        for slot in (-2, max(S().FIELD_IDS.values()) + 1, 1000):
            assert S().lib.sf_set_obstacles(fs._h, slot) == invalid
        assert fs.obstacles()["enabled"] == 0
        obstacles_on(fs, mask)
        assert S().lib.sf_set_obstacles(fs._h, -2) == invalid
        assert fs.obstacles()["enabled"] == 1  # unchanged
        upload_all(fs, random_fields(N, dtype, 80))
        with pytest.raises(S().SfError) as e:  # vel_step's default solver is the Jacobi one
            fs.vel_step()
        assert e.value.status == invalid and "SF_PRESSURE_CG" in str(e.value)
        fs.set_pressure_solver("cg", 1e-2, 5)
        fs.vel_step()
        fs.set_pressure_multigrid(2)
        for call in (fs.vel_step, lambda: fs.project_cg("u", "v", "w", "u0", "v0", 1e-2, 5)):
            with pytest.raises(S().SfError) as e:
                call()
            assert e.value.status == invalid and "multigrid" in str(e.value)
        fs.set_pressure_multigrid(0)
        fs.project_cg("u", "v", "w", "u0", "v0", 1e-2, 5)
        fs.set_obstacles(None)
        fs.set_pressure_multigrid(2)
        fs.project_cg("u", "v", "w", "u0", "v0", 1e-2, 5)  # multigrid without obstacles: as before
