"""MacCormack under the mask on the device (docs/SPEC.md §18, sf_set_obstacle_maccormack): everything is held to the
bits of tests/obstacle_maccormack_ref.py on the masks of tests/obstacle_cases.py and the inputs of
tests/obstacle_maccormack_cases.py.

(a) sf_advect_maccormack_masked under every mask family at every size class, both precisions, b = 0 .. 3, on inputs
    whose stored shells are independent random numbers, once more with a NaN parked in every solid cell, and on the
    `specials` inputs under `box`;
(b) four decompositions over each of the two transports, `box` and `random30`; a reverse trace past the stored ghost
    planes is SF_ERR_HALO_EXCEEDED;
(c) vel_step + dens_step with the setting on (the three-field form) against the step composed in numpy: every size class,
    both precisions, the three mixed scheme pairs, bound sources with forces, the masked V-cycle, two slabs;
(d) SF_GRAPH=1 around switching the setting;
(e) with the setting off the launches of a §17 step and of a §15 + MacCormack step are those of a context that never
    set it;
(f) the refusals.
tests/test_obstacle_maccormack_ref.py shows on the CPU which wrong readings of §18 these cases tell from the right one.
The schedule-hazard check of tests/conftest.py reads the trace of every context created here."""
import os

import numpy as np
import pytest

import obstacle_cases as OC
import obstacle_maccormack_cases as MC
import obstacle_maccormack_ref as MM
import obstacle_transport_ref as TR
import obstacles_mg_ref as OM
import obstacles_ref as OB
import shape_cases as C
from gpu_support import DIFF, DT, USER, VISC, S, assert_same_bits, make, random_fields, set_forces, slab0_ops, upload_all

pytestmark = pytest.mark.gpu

MASK_SLOT = "v0"  # a slot no single operator below touches


def masked_on(fs, mask, slot=MASK_SLOT, maccormack=None, first=False):
    """Obstacles and the setting of §17; maccormack: the setting of §18, before (first) or after them."""
    if maccormack is not None and first:
        fs.set_obstacle_maccormack(maccormack)
    fs.set_obstacles(mask, slot=slot)
    fs.fill(slot, float("nan"))  # the mask is read once
    fs.set_obstacle_transport(True)
    if maccormack is not None and not first:
        fs.set_obstacle_maccormack(maccormack)
    if maccormack is not None:
        assert fs.obstacle_maccormack() is bool(maccormack)


def check_operator(fs, d0, b, want, what, nan_ok=False):
    fs.upload("u0", d0)
    fs.fill("dens", float("nan"))  # every entry of the result is written
    fs.advect_maccormack_masked(b, "dens", "u0", "u", "v", "w")
    fs.sync()
    assert_same_bits(fs.download("dens"), want, f"{what}: advect_maccormack_masked b={b}", nan_ok=nan_ok)
    assert_same_bits(fs.download("u0"), d0, f"{what}: d0 is left alone", nan_ok=True)


# ---- (a) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,N,dtype", MC.OPERATORS, ids=[f"{f}-N{n}-{C.dname(t)}" for f, n, t in MC.OPERATORS])
def test_the_operator_under_every_family(family, N, dtype):
    """The setting of §18 governs the steps only: the operator runs with it unset (odd N) and set (even N)."""
    mask = OC.mask(family, N, dtype)
    solid = OB.Mask(mask).solid
    what = f"{family} N={N} {C.dname(dtype)}"
    with make(N, dtype) as fs:
        masked_on(fs, mask, maccormack=None if N % 2 else True, first=N % 4 == 0)
        for n, a in zip(("u", "v", "w"), MC.inputs(family, N, dtype, 0)[1]):
            fs.upload(n, a)
        for b in MC.BS:
            d0 = MC.inputs(family, N, dtype, b)[0]
            want = MC.want(family, N, dtype, b)
            check_operator(fs, d0, b, want, what)
            check_operator(fs, OC.parked_nan((d0,), solid)[0], b, want, what + " NaN in the solids")
        if family == "box" and N >= 13:
            got = fs.download("dens")[1:-1, 1:-1, 1:-1]
            assert not got[solid].any() and got[~solid].any()


@pytest.mark.parametrize("N,dtype", MC.SPECIALS, ids=[f"N{n}-{C.dname(t)}" for n, t in MC.SPECIALS])
def test_the_operator_on_special_inputs(N, dtype):
    mask = OC.mask("box", N, dtype)
    with make(N, dtype) as fs:
        masked_on(fs, mask)
        for b in MC.BS:
            d0, vel = MC.special_inputs(N, dtype, b)
            for n, a in zip(("u", "v", "w"), vel):
                fs.upload(n, a)
            check_operator(fs, d0, b, MC.want_special(N, dtype, b), f"specials box N={N} {C.dname(dtype)}", nan_ok=True)


# ---- (b) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,N,P,transport", MC.DECOMPOSED, ids=[f"{f}-N{n}-P{p}-{tr}" for f, n, p, tr in MC.DECOMPOSED])
def test_every_decomposition(family, N, P, transport):
    """The P = 1 reference: hat's ghost planes are exchanged between the passes, and the reverse trace of a slab's first
    and last plane takes hat and the solidity of its samples from the ghost planes."""
    dtype = MC.decomposed_dtype(P)
    mask = OC.mask(family, N, dtype, P)
    what = f"{family} N={N} P={P} {transport}"
    with make(N, dtype, P=P, transport=transport) as fs:
        masked_on(fs, mask)
        for n, a in zip(("u", "v", "w"), MC.inputs(family, N, dtype, 0, True)[1]):
            fs.upload(n, a)
        for b in MC.BS:
            check_operator(fs, MC.inputs(family, N, dtype, b, True)[0], b, MC.want(family, N, dtype, b, True, P), what)
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


def test_a_reverse_trace_past_the_ghost_planes_is_reported():
    N, P, dtype = 34, 2, np.float32
    mask = OC.mask("random30", N, dtype, P)
    assert OB.Mask(mask).fluid[N // 2 - 1, N // 2 - 1, N // 2 - 1]  # the cell with the long trace is a fluid cell
    with make(N, dtype, P=P) as fs:
        masked_on(fs, mask)
        for n, a in zip(("u", "v", "w"), MC.far_reverse_velocity("random30", N, dtype)):
            fs.upload(n, a)
        fs.upload("u0", MC.inputs("random30", N, dtype, 0)[0])
        fs.advect_masked(0, "dens", "u0", "u", "v", "w")  # the forward trace alone stays inside
        fs.sync()
        fs.advect_maccormack_masked(0, "dens", "u0", "u", "v", "w")
        with pytest.raises(S().SfError) as e:
            fs.sync()
        assert e.value.status == S().SF_ERR_HALO_EXCEEDED
        fs.sync()  # the flag is cleared once reported


# ---- (c) -----------------------------------------------------------------------------------------------------------
STEP_TOL, STEP_ITERS, STEP_K = 1e-2, 4, 2
FORCES = dict(eps=0.3, beta=0.5, ambient=0.1, axis=1)
SMALL_MASKS = {1: "walls", 2: "random30", 3: "walls", 5: "random30"}
NAMES = {MC.MC: "MC", MC.SL: "SL"}
# (N, dtype, schemes, solver, bound sources and forces, P, transport)
STEPS = ([(N, t, s, "cg", False, 1, "copy") for N in MC.SIZES for t in C.DTYPES for s in MC.SCHEMES]
         + [(13, np.float64, MC.SCHEMES[0], "cg", True, 1, "copy"), (34, np.float32, MC.SCHEMES[0], "mg", False, 1, "copy"),
            (34, np.float32, MC.SCHEMES[0], "cg", False, 2, "copy"), (34, np.float64, MC.SCHEMES[1], "cg", True, 2, "rccl-self"),
            (34, np.float32, MC.SCHEMES[2], "cg", False, 2, "rccl-self")])
MG = (2, 0, 8)


def step_mask(N, dtype):
    return OC.mask("box" if N >= 13 else SMALL_MASKS[N], N, dtype)


def step_fields(N, dtype, P):
    """Traces of a third of a cell (sigma) on one slab; within one plane on two."""
    return random_fields(N, dtype, 181, vel=0.05 if P > 1 else 0.3 / (DT * N))


def step_reference(N, dtype, schemes, solver, bound, P):
    """One vel_step + dens_step composed from the references."""
    def build():
        f = step_fields(N, dtype, P)
        mask = step_mask(N, dtype)
        if solver == "mg":
            project = lambda u, v, w: OM.project_cg(u, v, w, mask, STEP_TOL, STEP_ITERS, *MG)  # noqa: E731
        else:
            project = lambda u, v, w: OB.project_cg(u, v, w, mask, STEP_TOL, STEP_ITERS, 0)  # noqa: E731
        src = {n: f[n] for n in ("u0", "v0", "w0")} if bound else None
        vel = MM.vel_step(f, mask, STEP_K, DT, VISC, project, sources=src, forces=FORCES if bound else None,
                          scheme=schemes[0])
        dens = MM.dens_step(f["dens"], f["dens0"], vel["u"], vel["v"], vel["w"], mask, STEP_K, DT, DIFF, scheme=schemes[1])
        return vel, dens
    return MC.once(("step", N, C.dname(dtype), schemes, solver, bound, P), build)


@pytest.mark.parametrize("N,dtype,schemes,solver,bound,P,transport", STEPS,
                         ids=[f"N{n}-{C.dname(t)}-{NAMES[s[0]]}{NAMES[s[1]]}-{sv}-{'bound-forces' if b else 'plain'}-P{p}-{tr}"
                              for n, t, s, sv, b, p, tr in STEPS])
def test_steps_with_the_setting_on(N, dtype, schemes, solver, bound, P, transport):
    f = step_fields(N, dtype, P)
    mask = step_mask(N, dtype)
    vel, dens = step_reference(N, dtype, schemes, solver, bound, P)
    solid = OB.Mask(mask).solid
    what = f"N={N} {C.dname(dtype)} {schemes} {solver} bound={bound} P={P} {transport}"
    MC.check_nan_share({"u": vel["u"], "v": vel["v"], "w": vel["w"], "dens": dens}, mask, what)
    with make(N, dtype, K=STEP_K, P=P, transport=transport) as fs:
        fs.set_pressure_solver("cg", STEP_TOL, STEP_ITERS)
        if solver == "mg":
            fs.set_pressure_multigrid(*MG)
            fs.set_obstacle_multigrid(True)
        if bound:
            set_forces(fs, **FORCES)
        fs.set_advection(*schemes)
        masked_on(fs, mask, slot="u0", maccormack=True, first=N % 2 == 0)
        upload_all(fs, f)
        if bound:
            for n, slot in USER.items():
                fs.upload(slot, f[n])
            fs.bind_sources()
        fs.vel_step()
        info = fs.pressure_info()
        print(f"{what}: {info}")
        assert (info["status"], info["iterations"]) == (vel["status"], vel["iterations"])
        fs.dens_step()
        fs.sync()
        for n in ("u", "v", "w"):
            assert_same_bits(fs.download(n), vel[n], f"{what}: {n}")
        got = fs.download("dens")
        assert_same_bits(got, dens, f"{what}: dens")
        assert not got[1:-1, 1:-1, 1:-1][solid].any()


# ---- (d) -----------------------------------------------------------------------------------------------------------
def test_graphs_around_switching_the_setting(monkeypatch):
    """dens_step under SF_GRAPH=1 on one slab: MacCormack with the setting on three times, first order with it off
    twice, MacCormack with it on again twice: the bits of the run without graphs, so no cached graph of one form is
    replayed for the other, and the steps are §18's and §17's."""
    N, dtype, K = 34, np.float32, 4
    f = random_fields(N, dtype, 182)
    mask = OC.mask("box", N, dtype)
    sequence = (True, True, True, False, False, True, True)
    Sx = S()
    runs = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("SF_GRAPH", graph)
        got = []
        with make(N, dtype, K=K) as fs:
            upload_all(fs, f)
            masked_on(fs, mask, slot="u0")
            for on in sequence:
                if on != fs.obstacle_maccormack():
                    fs.set_advection(Sx.SF_ADVECT_SEMI_LAGRANGIAN, Sx.SF_ADVECT_MACCORMACK if on else Sx.SF_ADVECT_SEMI_LAGRANGIAN)
                    fs.set_obstacle_maccormack(on)
                fs.upload("dens0", f["dens0"])
                fs.dens_step()
                fs.sync()
                got.append(fs.download("dens"))
        runs[graph] = got
    for step, (a, b) in enumerate(zip(runs["0"], runs["1"])):
        assert_same_bits(b, a, f"dens_step {step} with graphs")
    vel = [f[n] for n in ("u", "v", "w")]
    got = runs["1"]
    assert_same_bits(got[0], MM.dens_step(f["dens"], f["dens0"], *vel, mask, K, DT, DIFF), "the first step: §18")
    assert_same_bits(got[2], MM.dens_step(got[1], f["dens0"], *vel, mask, K, DT, DIFF), "the third step: §18")
    assert_same_bits(got[3], TR.dens_step(got[2], f["dens0"], *vel, mask, K, DT, DIFF), "the step after switching off: §17")
    assert_same_bits(got[5], MM.dens_step(got[4], f["dens0"], *vel, mask, K, DT, DIFF), "the step after switching on again: §18")


# ---- (e) -----------------------------------------------------------------------------------------------------------
def renumbered(ops):
    """Op records with their buffers numbered by first appearance in the stretch."""
    ids, out = {}, []
    for op in ops:
        acc = [[a[0], ids.setdefault(a[1], len(ids)), a[2], a[3]] for a in op["acc"]]
        out.append((op["name"], op["stream"], acc))
    return out


@pytest.mark.parametrize("kind", ["transport", "maccormack"])
@pytest.mark.parametrize("P", [1, 2], ids=["P1", "P2"])
def test_the_setting_off_leaves_the_launches(P, kind):
    """A §17 step (transport: masked transport, first order) and a §15 step advected with MacCormack (maccormack:
    transport off) of a context that ran a §18 step before and switched the setting off, and of one that never set it:
    the same launches on the same planes, the same bits."""
    N, dtype = 34, np.float32
    path = os.environ["SF_TRACE_SCHEDULE"]
    Sx = S()
    f = random_fields(N, dtype, 183)
    mask = OC.mask("box", N, dtype, P)
    mc, sl = Sx.SF_ADVECT_MACCORMACK, Sx.SF_ADVECT_SEMI_LAGRANGIAN
    stretches, results = [], []
    for ever_set in (False, True):
        with make(N, dtype, K=4, P=P) as fs:
            fs.set_pressure_solver("cg", 1e-2, 5)
            fs.set_pressure_preconditioner("jacobi", 2)
            masked_on(fs, mask, slot="u0")
            if ever_set:
                fs.set_obstacle_maccormack(True)
                fs.set_advection(mc, mc)
                upload_all(fs, f)
                fs.vel_step()
                fs.dens_step()
                fs.set_obstacle_maccormack(False)
                assert fs.obstacle_maccormack() is False
            if kind == "transport":
                fs.set_advection(sl, sl)
            else:
                fs.set_advection(mc, mc)
                fs.set_obstacle_transport(False)
            fs.sync()
            start = len(slab0_ops(path))
            upload_all(fs, f)
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            stretches.append(renumbered(slab0_ops(path)[start:]))
            results.append({n: fs.download(n) for n in ("u", "v", "w", "dens")})
    names = [name for name, _, _ in stretches[1]]
    assert len(names) > 20 and "advect_mc_masked" not in names
    assert ("advect_masked" in names) == (kind == "transport") and ("advect_mc" in names) == (kind == "maccormack")
    assert stretches[0] == stretches[1]
    for n, a in results[0].items():
        assert_same_bits(results[1][n], a, n)


# ---- (f) -----------------------------------------------------------------------------------------------------------
def test_refusals():
    N, dtype = 13, np.float32
    mask = OC.mask("box", N, dtype)
    Sx = S()
    invalid = Sx.SF_ERR_INVALID
    op = lambda fs: fs.advect_maccormack_masked(0, "dens", "u0", "u", "v", "w")  # noqa: E731
    with make(N, dtype) as fs:
        upload_all(fs, random_fields(N, dtype, 184))
        for value in (2, -1):
            assert Sx.lib.sf_set_obstacle_maccormack(fs._h, value) == invalid
            assert fs.obstacle_maccormack() is False  # unchanged
        fs.set_obstacle_maccormack(True)
        for value in (2, -1):
            assert Sx.lib.sf_set_obstacle_maccormack(fs._h, value) == invalid
            assert fs.obstacle_maccormack() is True  # unchanged
        for transport in (False, True):  # obstacles off: refused whatever the settings
            fs.set_obstacle_transport(transport)
            with pytest.raises(Sx.SfError) as e:
                op(fs)
            assert e.value.status == invalid and "sf_set_obstacles" in str(e.value)
        fs.set_obstacles(mask, slot=MASK_SLOT)
        op(fs)
        fs.set_obstacle_transport(False)  # obstacles on, transport off: refused, the setting of §18 does not replace it
        with pytest.raises(Sx.SfError) as e:
            op(fs)
        assert e.value.status == invalid and "sf_set_obstacle_transport" in str(e.value)
        fs.set_obstacle_transport(True)
        for args in ((0, "u0", "u0", "u", "v", "w"), (0, "u", "u0", "u", "v", "w"), (0, "v", "u0", "u", "v", "w"),
                     (0, "w", "u0", "u", "v", "w")):  # an aliased output
            with pytest.raises(Sx.SfError) as e:
                fs.advect_maccormack_masked(*args)
            assert e.value.status == invalid
        # the setting off: both steps still refuse with a message; the operator singly does not depend on it
        fs.set_obstacle_maccormack(False)
        op(fs)
        fs.set_pressure_solver("cg", 1e-2, 5)
        fs.set_advection(Sx.SF_ADVECT_MACCORMACK, Sx.SF_ADVECT_MACCORMACK)
        for step in (fs.vel_step, fs.dens_step):
            with pytest.raises(Sx.SfError) as e:
                step()
            assert e.value.status == invalid and "MacCormack" in str(e.value)
        fs.set_obstacle_maccormack(True)
        fs.vel_step()
        fs.dens_step()
        fs.sync()
