"""Mask-aware transport on the device (docs/SPEC.md §17, sf_set_obstacle_transport): everything is held to the bits of
tests/obstacle_transport_ref.py on the masks of tests/obstacle_cases.py and the inputs of
tests/obstacle_transport_cases.py.

(a) sf_diffuse_masked (K = 1, 2, 5) and sf_advect_masked under every mask family at every size class, both precisions,
    b = 0 .. 3, on inputs whose stored shells are independent random numbers, and once more with a NaN parked in every
    solid cell of every input;
(b) the sweep at the row shapes whose lanes take a second trip or end in a ragged vector;
(c) four decompositions over each of the two transports, walls (solids on both sides of every slab boundary) and
    random30; a back-trace past the stored ghost planes is SF_ERR_HALO_EXCEEDED;
(d) two vel_step + dens_step against the step composed in numpy: plain CG, jacobi:2 and the masked V-cycle, bound and
    unbound sources, forces, one slab and two, the scalars on the host and on the device;
(e) SF_GRAPH=1 around switching the setting on and off, with an even and an odd K, and the §15 step after switching off;
(f) switching the setting off restores the launches of a context that never set it;
(g) the refusals.
tests/test_obstacle_transport_ref.py shows on the CPU which wrong readings of §17 these cases tell from the right one.
The schedule-hazard check of tests/conftest.py reads the trace of every context created here."""
import os
import time

import numpy as np
import pytest

import obstacle_cases as OC
import obstacle_transport_cases as TC
import obstacle_transport_ref as TR
import obstacles_mg_ref as OM
import obstacles_ref as OB
import shape_cases as C
from gpu_support import DIFF, DT, USER, VISC, S, assert_same_bits, make, random_fields, set_forces, slab0_ops, upload_all

pytestmark = pytest.mark.gpu

MASK_SLOT = "v0"  # a slot no single operator below touches
_WANT = {}


def transport_on(fs, mask, slot=MASK_SLOT, order="obstacles first"):
    """Obstacles and the setting of §17, in either order."""
    assert fs.obstacle_transport() is False
    if order != "obstacles first":
        fs.set_obstacle_transport(True)
    fs.set_obstacles(mask, slot=slot)
    fs.fill(slot, float("nan"))  # the mask is read once
    if order == "obstacles first":
        fs.set_obstacle_transport(True)
    assert fs.obstacle_transport() is True


def once(key, build):
    """A reference computed once per case and only read afterwards."""
    if key not in _WANT:
        t0 = time.perf_counter()
        _WANT[key] = build()
        if time.perf_counter() - t0 > 0.5:
            print(f"reference {key}: {time.perf_counter() - t0:.1f} s")
    return _WANT[key]


def want_diffuse(family, N, dtype, b, K, P=None):
    def build():
        x, x0 = TC.fields(family, N, dtype, b)
        TR.diffuse_masked(b, x, x0, TC.DIFF, DT, K, OC.mask(family, N, dtype, P))
        return x
    return once(("diffuse", family, N, C.dname(dtype), b, K, P), build)


def want_advect(family, N, dtype, b, one_plane=False, P=None):
    def build():
        d0 = TC.fields(family, N, dtype, b)[1]
        d = np.zeros_like(d0)
        TR.advect_masked(b, d, d0, *TC.velocity(family, N, dtype, one_plane), DT, OC.mask(family, N, dtype, P))
        return d
    return once(("advect", family, N, C.dname(dtype), b, one_plane, P), build)


def check_diffuse(fs, family, N, dtype, b, K, want, what, parked=None):
    x, x0 = TC.fields(family, N, dtype, b)
    if parked is not None:
        x, x0 = OC.parked_nan((x, x0), parked)
    fs.set_iters(K)
    fs.upload("dens", x)
    fs.upload("u0", x0)
    fs.diffuse_masked(b, "dens", "u0", TC.DIFF)
    fs.sync()
    assert_same_bits(fs.download("dens"), want, f"{what}: diffuse_masked b={b} K={K}")
    assert_same_bits(fs.download("u0"), x0, f"{what}: x0 is left alone", nan_ok=True)


def check_advect(fs, family, N, dtype, b, want, what, one_plane=False, parked=None):
    d0 = TC.fields(family, N, dtype, b)[1]
    if parked is not None:
        d0 = OC.parked_nan((d0,), parked)[0]
    fs.upload("u0", d0)
    fs.fill("dens", float("nan"))  # every entry of the result is written
    fs.advect_masked(b, "dens", "u0", "u", "v", "w")
    fs.sync()
    assert_same_bits(fs.download("dens"), want, f"{what}: advect_masked b={b}")


# ---- (a) -----------------------------------------------------------------------------------------------------------
OPERATORS = [(f, N, t) for f in TC.FAMILIES for N in TC.SIZES for t in C.DTYPES]


@pytest.mark.parametrize("family,N,dtype", OPERATORS, ids=[f"{f}-N{n}-{C.dname(t)}" for f, n, t in OPERATORS])
def test_single_operators_under_every_family(family, N, dtype):
    mask = OC.mask(family, N, dtype)
    solid = OB.Mask(mask).solid
    what = f"{family} N={N} {C.dname(dtype)}"
    with make(N, dtype) as fs:
        transport_on(fs, mask, order="obstacles first" if N % 2 else "setting first")
        assert fs.obstacles()["fluid_cells"] == int((~solid).sum())
        for n, a in zip(("u", "v", "w"), TC.velocity(family, N, dtype)):
            fs.upload(n, a)
        for b in TC.BS:
            for K in TC.SWEEPS:
                check_diffuse(fs, family, N, dtype, b, K, want_diffuse(family, N, dtype, b, K), what)
            check_diffuse(fs, family, N, dtype, b, 2, want_diffuse(family, N, dtype, b, 2), what + " NaN in the solids", solid)
            check_advect(fs, family, N, dtype, b, want_advect(family, N, dtype, b), what)
            check_advect(fs, family, N, dtype, b, want_advect(family, N, dtype, b), what + " NaN in the solids", parked=solid)
        if family == "box" and N >= 13:
            got = fs.download("dens")[1:-1, 1:-1, 1:-1]
            assert not got[solid].any() and got[~solid].any()


def test_no_sweep_is_a_no_op():
    N, dtype = 13, np.float32
    x, x0 = TC.fields("box", N, dtype)
    with make(N, dtype, K=0) as fs:
        transport_on(fs, OC.mask("box", N, dtype))
        fs.upload("dens", x)
        fs.upload("u0", x0)
        fs.diffuse_masked(0, "dens", "u0", TC.DIFF)
        fs.sync()
        assert_same_bits(fs.download("dens"), x, "K = 0")


# ---- (b) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype,K", TC.ROW_SHAPES, ids=[f"N{n}-{C.dname(t)}-K{k}" for n, t, k in TC.ROW_SHAPES])
def test_row_shapes_of_the_sweep(N, dtype, K):
    """random30; one b per size (N mod 4), so the four are spread over the shapes."""
    b = N % 4
    with make(N, dtype) as fs:
        transport_on(fs, OC.mask("random30", N, dtype))
        check_diffuse(fs, "random30", N, dtype, b, K, want_diffuse("random30", N, dtype, b, K), f"random30 N={N}")


# ---- (c) -----------------------------------------------------------------------------------------------------------
DECOMPOSED = [(f, N, P, tr) for N, P in TC.DECOMPOSED for f in ("walls", "random30") for tr in ("copy", "rccl-self")]


@pytest.mark.parametrize("family,N,P,transport", DECOMPOSED, ids=[f"{f}-N{n}-P{p}-{tr}" for f, n, p, tr in DECOMPOSED])
def test_every_decomposition(family, N, P, transport):
    """The P = 1 reference. The walls mask has solid cells on both sides of every boundary of these P slabs, so the
    samples of a slab's first and last plane take their solidity from the ghost planes of the face codes."""
    dtype = np.float32 if P != 17 else np.float64
    mask = OC.mask(family, N, dtype, P)
    what = f"{family} N={N} P={P} {transport}"
    with make(N, dtype, P=P, transport=transport) as fs:
        transport_on(fs, mask, order="setting first" if transport == "copy" else "obstacles first")
        for n, a in zip(("u", "v", "w"), TC.velocity(family, N, dtype, one_plane=True)):
            fs.upload(n, a)
        for b in TC.BS:
            check_diffuse(fs, family, N, dtype, b, 5, want_diffuse(family, N, dtype, b, 5, P), what)
            check_advect(fs, family, N, dtype, b, want_advect(family, N, dtype, b, True, P), what, one_plane=True)
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


def test_a_trace_past_the_ghost_planes_is_reported():
    N, P, dtype = 34, 2, np.float32
    with make(N, dtype, P=P) as fs:
        transport_on(fs, OC.mask("walls", N, dtype, P))
        for n, a in zip(("u", "v", "w"), TC.far_velocity("walls", N, dtype)):
            fs.upload(n, a)
        fs.upload("u0", TC.fields("walls", N, dtype)[1])
        fs.advect_masked(0, "dens", "u0", "u", "v", "w")
        with pytest.raises(S().SfError) as e:
            fs.sync()
        assert e.value.status == S().SF_ERR_HALO_EXCEEDED
        fs.sync()  # the flag is cleared once reported


# ---- (d) -----------------------------------------------------------------------------------------------------------
STEP_TOL, STEP_ITERS, STEP_K = 1e-2, 10, 4
FORCES = dict(eps=0.3, beta=0.5, ambient=0.1, axis=1)
SOLVERS = {"cg": ("jacobi", 0, None), "jacobi2": ("jacobi", 2, None), "mg": (None, 0, (2, 0, 8)), "mg1": (None, 0, (2, 1, 8))}
# (N, solver, bound sources, forces, P, check_every): every solver with and without bound sources and forces; two slabs
# and the device scalars spread over them (mg1: the one-level cycle, the depth two slabs of 17 planes admit)
STEPS = ([(13, s, bound, bound, 1, 4 if bound else 0) for s in ("cg", "jacobi2", "mg") for bound in (False, True)]
         + [(34, s, *c) for s in ("cg", "jacobi2")
            for c in ((False, False, 1, 0), (True, False, 2, 4), (False, True, 2, 0), (True, True, 1, 4))]
         + [(34, "mg", False, False, 1, 0), (34, "mg", True, True, 1, 4), (34, "mg1", True, False, 2, 4),
            (34, "mg1", False, True, 2, 0)])


def step_dtype(N):
    return np.float64 if N == 13 else np.float32


def step_reference(N, solver, bound, forces):
    """Two vel_step + dens_step composed from the references; the x0 slots hold the sources again before each step."""
    def build():
        dtype = step_dtype(N)
        f = random_fields(N, dtype, 177)
        mask = OC.mask("box", N, dtype)
        _, m, mg = SOLVERS[solver]
        if mg:
            project = lambda u, v, w: OM.project_cg(u, v, w, mask, STEP_TOL, STEP_ITERS, *mg)  # noqa: E731
        else:
            project = lambda u, v, w: OB.project_cg(u, v, w, mask, STEP_TOL, STEP_ITERS, m)  # noqa: E731
        g, outs = dict(f), []
        src = {n: f[n] for n in ("u0", "v0", "w0")} if bound else None
        for _ in range(2):
            vel = TR.vel_step(g, mask, STEP_K, DT, VISC, project, sources=src, forces=FORCES if forces else None)
            dens = TR.dens_step(g["dens"], f["dens0"], vel["u"], vel["v"], vel["w"], mask, STEP_K, DT, DIFF)
            outs.append((vel, dens))
            g = dict(f, u=vel["u"], v=vel["v"], w=vel["w"], dens=dens)
        return outs
    return once(("steps", N, solver, bound, forces), build)


@pytest.mark.parametrize("N,solver,bound,forces,P,every", STEPS,
                         ids=[f"N{n}-{s}-{'bound' if b else 'unbound'}-{'forces' if f else 'plain'}-P{p}-sync{e}"
                              for n, s, b, f, p, e in STEPS])
def test_steps_with_a_box(N, solver, bound, forces, P, every):
    dtype = step_dtype(N)
    f = random_fields(N, dtype, 177)
    mask = OC.mask("box", N, dtype)
    outs = step_reference(N, solver, bound, forces)
    solid = OB.Mask(mask).solid
    kind, m, mg = SOLVERS[solver]
    what = f"N={N} {solver} bound={bound} forces={forces} P={P} sync={every}"
    with make(N, dtype, K=STEP_K, P=P, transport="rccl-self" if bound else "copy") as fs:
        fs.set_pressure_solver("cg", STEP_TOL, STEP_ITERS)
        fs.set_pressure_sync(every)
        if mg:
            fs.set_pressure_multigrid(*mg)
            fs.set_obstacle_multigrid(True)
        else:
            fs.set_pressure_preconditioner("jacobi" if m else "none", m)
        if forces:
            set_forces(fs, **FORCES)
        transport_on(fs, mask, slot="u0")  # (every user slot may be bound: a slot that is scratch before the first step)
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
            assert vel["iterations"] >= 1
            fs.dens_step()
            fs.sync()
            for n in ("u", "v", "w"):
                assert_same_bits(fs.download(n), vel[n], f"{what} step {step}: {n}")
            got = fs.download("dens")
            assert_same_bits(got, dens, f"{what} step {step}: dens")
            assert not got[1:-1, 1:-1, 1:-1][solid].any() and got[1:-1, 1:-1, 1:-1][~solid].any()
            if not bound:
                for n in ("u0", "v0", "w0", "dens0"):
                    fs.upload(n, f[n])


# ---- (e) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 5], ids=["K4", "K5"])
def test_graphs_around_switching_the_setting(monkeypatch, K):
    """dens_step with the setting on four times, off twice, on, off under SF_GRAPH=1: the bits of the run without graphs,
    so no cached graph of one form is replayed for the other; the first step is §17's, the first one after switching off
    §15's on the density the step before left. K = 5: every masked solve leaves the slot and its scratch partner
    exchanged (one swap per sweep), so the repeated steps meet the pointer states the graph cache keys on. Only
    dens_step is sequenced: vel_step with the CG solver, which obstacles need, is never captured."""
    N, dtype = 34, np.float32
    f = random_fields(N, dtype, 178)
    mask = OC.mask("box", N, dtype)
    sequence = (True, True, True, True, False, False, True, False)
    runs = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("SF_GRAPH", graph)
        got = []
        with make(N, dtype, K=K) as fs:
            upload_all(fs, f)
            fs.set_obstacles(mask, slot="u0")
            for on in sequence:
                if on != fs.obstacle_transport():
                    fs.set_obstacle_transport(on)
                fs.upload("dens0", f["dens0"])
                fs.dens_step()
                fs.sync()
                got.append(fs.download("dens"))
        runs[graph] = got
    for step, (a, b) in enumerate(zip(runs["0"], runs["1"])):
        assert_same_bits(b, a, f"dens_step {step} with graphs")
    vel = [f[n] for n in ("u", "v", "w")]
    got = runs["1"]
    assert_same_bits(got[0], TR.dens_step(f["dens"], f["dens0"], *vel, mask, K, DT, DIFF), "the first step: §17")
    assert_same_bits(got[3], TR.dens_step(got[2], f["dens0"], *vel, mask, K, DT, DIFF), "the fourth step: §17")
    assert_same_bits(got[4], OB.dens_step(got[3], f["dens0"], *vel, mask, K, DT, DIFF), "the step after switching off: §15")
    assert_same_bits(got[6], TR.dens_step(got[5], f["dens0"], *vel, mask, K, DT, DIFF), "the step after switching on again: §17")


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
    """A §15 step (obstacles on) of a context that had the setting on for a step, and of one that never had: the same
    launches on the same planes, the same bits; sf_set_obstacles launches nothing more than before either."""
    N, dtype = 34, np.float32
    path = os.environ["SF_TRACE_SCHEDULE"]
    f = random_fields(N, dtype, 179)
    mask = OC.mask("box", N, dtype, P)
    stretches, results = [], []
    for ever_set in (False, True):
        with make(N, dtype, K=4, P=P) as fs:
            fs.set_pressure_solver("cg", 1e-2, 5)
            fs.set_pressure_preconditioner("jacobi", 2)
            if ever_set:
                transport_on(fs, mask, slot="u0")
                upload_all(fs, f)
                fs.vel_step()
                fs.dens_step()
                fs.set_obstacle_transport(False)
                assert fs.obstacle_transport() is False
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
    assert len(names) > 20 and "zero_solid" in names and "face_code" in names
    assert not any(name in ("lin_solve_masked", "advect_masked", "code_shells") for name in names)
    assert stretches[0] == stretches[1]
    for n, a in results[0].items():
        assert_same_bits(results[1][n], a, n)


# ---- (g) -----------------------------------------------------------------------------------------------------------
def test_refusals():
    N, dtype = 13, np.float32
    mask = OC.mask("box", N, dtype)
    Sx = S()
    invalid = Sx.SF_ERR_INVALID
    ops = (lambda fs: fs.diffuse_masked(0, "dens", "u0", DIFF), lambda fs: fs.advect_masked(0, "dens", "u0", "u", "v", "w"))
    with make(N, dtype) as fs:
        upload_all(fs, random_fields(N, dtype, 180))
        for value in (2, -1, 7):
            assert Sx.lib.sf_set_obstacle_transport(fs._h, value) == invalid
            assert fs.obstacle_transport() is False  # unchanged
        for setting in (False, True):  # obstacles off: refused whatever the setting
            fs.set_obstacle_transport(setting)
            for op in ops:
                with pytest.raises(Sx.SfError) as e:
                    op(fs)
                assert e.value.status == invalid and "sf_set_obstacles" in str(e.value)
        assert Sx.lib.sf_set_obstacle_transport(fs._h, 2) == invalid
        assert fs.obstacle_transport() is True  # unchanged
        fs.set_obstacles(mask, slot=MASK_SLOT)
        for op in ops:
            op(fs)
        fs.set_obstacle_transport(False)  # obstacles on, the setting off: refused
        for op in ops:
            with pytest.raises(Sx.SfError) as e:
                op(fs)
            assert e.value.status == invalid
        fs.set_obstacle_transport(True)
        with pytest.raises(Sx.SfError) as e:  # aliasing as the siblings
            fs.diffuse_masked(0, "dens", "dens", DIFF)
        assert e.value.status == invalid
        with pytest.raises(Sx.SfError) as e:
            fs.advect_masked(0, "u", "u0", "u", "v", "w")
        assert e.value.status == invalid
        # MacCormack with the setting on: both steps refused with a message, the setting and the scheme unchanged
        fs.set_pressure_solver("cg", 1e-2, 5)
        fs.set_advection(Sx.SF_ADVECT_MACCORMACK, Sx.SF_ADVECT_MACCORMACK)
        for step in (fs.vel_step, fs.dens_step):
            with pytest.raises(Sx.SfError) as e:
                step()
            assert e.value.status == invalid and "MacCormack" in str(e.value)
        assert fs.obstacle_transport() is True
        fs.set_advection(Sx.SF_ADVECT_MACCORMACK, Sx.SF_ADVECT_SEMI_LAGRANGIAN)
        fs.dens_step()  # the density's scheme alone decides dens_step
        with pytest.raises(Sx.SfError):
            fs.vel_step()
        fs.set_obstacle_transport(False)
        fs.vel_step()  # §15 with MacCormack: as before
        fs.sync()
