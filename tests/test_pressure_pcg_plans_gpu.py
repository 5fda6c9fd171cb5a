"""The preconditioned CG projection (docs/SPEC.md §11.2) under every pass plan, switch and slab depth. z = M(r) is
op_lin_solve, so its passes go through plan_solve, for_planes and the switches of any solve; what is the
preconditioner's own is host code — the ping-pong between two internal slots, the exchange of an internal slot, r's
ghost planes before the sweeps, the join in front of the row kernels, the memset of a z that is no implicit zero, two
more owning slots in the graph cache's key — and all of it depends on the passes the planner lays out. Every
comparison is in bits against tests/pressure_pcg_ref.py, which knows no switch; the schedule-hazard check of
tests/conftest.py reads the trace of every context created here.

(a) every pass plan of pcg_cases.PLANS on one slab, to convergence, scalars on the host and on the device;
(b) every pass plan on slabs (ghost zones of two and four planes, trapezoid blocks that grow, snap back and restart), six
    iterations, and one run to convergence per (N, P);
(c) in (a), (b) and (d) the plan of the case is read back from the schedule trace: the case ran the passes it is there for;
(d) the switches that change a plan, a kernel form or the schedule, each against the reference;
(e) vel_step with the preconditioner under the switch settings of the unpreconditioned CG step;
(f) MacCormack, forces, bound sources and jacobi:8 at once, against the step composed in numpy;
(g) graph replay around uncaptured preconditioned steps that leave z and its partner swapped, against no graphs.
tests/test_pressure_pcg_ref.py shows on the CPU that the table covers every pass kind and which of these inputs tell
stale ghost planes of r and of z from the reference."""
import os
import time

import numpy as np
import pytest

import diagnostics_ref as D
import maccormack_ref as MC
import pcg_cases as PC
import pressure_cg_ref as R
import pressure_pcg_ref as Q
import shape_cases as C
from gpu_support import (CG_STEP_SETTINGS, DIFF, DT, S, assert_same_bits, check_solve, make, passes_of_M, random_fields,
                         reference_vel_step, slab0_ops, traced_plans, upload_all)

pytestmark = pytest.mark.gpu

TOL = PC.TOL
TRACE_CAP = 64 << 20  # tests/conftest.py checks the hazards of a trace below this size only
_REFERENCES = {}


def reference(N, dtype, max_iters, m):
    """Q.project_cg of cg_velocity(N, dtype, PC.seed(N)): computed once per input, only read afterwards."""
    key = (N, C.dname(dtype), max_iters, m)
    if key not in _REFERENCES:
        t0 = time.perf_counter()
        _REFERENCES[key] = Q.project_cg(*C.cg_velocity(N, dtype, PC.seed(N)), TOL, max_iters, m)
        print(f"reference {key}: {time.perf_counter() - t0:.1f} s")
    return _REFERENCES[key]


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_plan(want_G, want_plan, tuned_case=None):
    """After the context is closed: the context of this test (the last one in the trace) ran, between every two r.z
    sums, exactly the passes of `want_plan` on `want_G` ghost planes, and its trace is small enough for the hazard
    check to run."""
    path = os.environ["SF_TRACE_SCHEDULE"].split(",")[0]
    size = os.path.getsize(path)
    assert size < TRACE_CAP, f"trace of {size} bytes: the schedule-hazard check would not run"
    ctx, plans = traced_plans(path)[-1]
    if tuned_case is not None:
        assert ctx["trap"] in (0, 2, 5), ctx
        want_G, want_plan = tuned_case.plan_at(ctx["trap"])
    print(f"trace {size} bytes, {len(plans)} applications of M: G={ctx['G']} trap={ctx['trap']} plan {sorted(set(plans))}")
    assert ctx["G"] == want_G, (ctx, want_G)
    assert plans and set(plans) == {want_plan}, (sorted(set(plans)), want_plan)


def solve_on(case, iters_and_syncs, monkeypatch):
    """The case's context; for every (max_iters, check_every) one solve against the reference."""
    set_env(monkeypatch, case.env)
    u, v, w = C.cg_velocity(case.N, case.dtype, PC.seed(case.N))
    with make(case.N, case.dtype, P=case.P, transport=case.transport) as fs:
        fs.set_pressure_preconditioner("jacobi", case.m)
        for max_iters, every in iters_and_syncs:
            want = reference(case.N, case.dtype, max_iters, case.m)
            if max_iters == PC.TO_CONVERGENCE:
                assert want["status"] == R.CONVERGED and want["iterations"] >= 4
            else:
                assert (want["status"], want["iterations"]) == (R.MAX_ITERS, max_iters)
            fs.set_pressure_sync(every)
            check_solve(fs, u, v, w, TOL, max_iters, f"{case.id} [{case.plan}] max_iters={max_iters} sync={every}", want=want)
        if case.transport == "rccl-self" and case.P > 1:
            assert fs.transport_info()["rccl_groups"] > 0
    check_plan(case.G, case.plan, case if case.tuned else None)


# ---- (a) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.ONE_SLAB, ids=[c.id for c in PC.ONE_SLAB])
def test_every_pass_plan_on_one_slab(case, monkeypatch):
    """To convergence on the host path and with check_every = 3 on the same context: pairs, three- and four-sweep
    marching passes after a pair and after the zero-iterate marching pass, a pair or a single sweep last, and the first
    pass of either kind on a z that was really zeroed (m = 1, SF_ZERO_SKIP=0), at a size every precision fuses."""
    solve_on(case, [(PC.TO_CONVERGENCE, 0), (PC.TO_CONVERGENCE, 3)], monkeypatch)


# ---- (b) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.ON_SLABS, ids=[c.id for c in PC.ON_SLABS])
def test_every_pass_plan_on_slabs(case, monkeypatch):
    """Six iterations of the P = 1 input with check_every 0 and 4. Ghost zones of four planes (two at 64 / 4), boundary
    launches that grow by up to eight planes, snap back and start a second block within one M(r); r's ghost planes
    travel before every M, z's after every pass, from whichever of the two internal buffers is the iterate."""
    solve_on(case, [(PC.DECOMPOSED_ITERS, 0), (PC.DECOMPOSED_ITERS, 4)], monkeypatch)


TO_CONVERGENCE = [c for c in PC.ON_SLABS if c.m == PC.CONVERGED_M and "SF_ZERO_SKIP" not in c.env and not c.tuned]


@pytest.mark.parametrize("case", TO_CONVERGENCE, ids=[c.id for c in TO_CONVERGENCE])
def test_slabs_to_convergence(case, monkeypatch):
    assert len({(c.N, c.P) for c in TO_CONVERGENCE}) == len({(c.N, c.P) for c in PC.ON_SLABS}) == 5
    solve_on(case, [(PC.TO_CONVERGENCE, 0)], monkeypatch)


# ---- (d) -----------------------------------------------------------------------------------------------------------
SWITCHES = ([{"SF_GHOST": g} for g in "123"] + [{"SF_TRAP": t} for t in "025"] + [{"SF_SK_S": s} for s in "23"]
            + [{"SF_SK_FIRST": "0"}, {"SF_ZERO_SKIP": "0"}, {"SF_FUSE2": "0"}, {"SF_ISHELL": "0"}, {"SF_ISHELL": "2"},
               {"SF_MARCH": "0"}, {"SF_SPLIT": "0"}, {"SF_HALO_STREAM": "1"}, {"SF_HALO_STREAM": "2"}, {"SF_NT": "0"},
               {"SF_NT": "1"}, {"SF_OVL": "0"}, {"SF_OVL": "2"},
               {"SF_MARCH": "0", "SF_TRAP": "3", "SF_HALO_STREAM": "2", "SF_SPLIT_FIELDS": "0"}])
SWITCH_CONTEXTS = [(64, np.float32, 1), (64, np.float32, 2), (40, np.float64, 2)]


def switch_cases():
    """Every setting on top of SF_MARCH_MINCELLS_K=0, and alone where that is another plan than the default switches
    give (without the marching kernel: another G, single sweeps, a stored zero, growth or none)."""
    out = []
    for N, dtype, P in SWITCH_CONTEXTS:
        for m in (8, 5):
            for env in SWITCHES:
                out.append((N, dtype, P, m, dict(PC.MARCH, **env)))
                if PC.model(N, dtype, P, m, env) != PC.model(N, dtype, P, m, {}):
                    out.append((N, dtype, P, m, env))
    return out


SWITCH_CASES = switch_cases()


def switch_id(c):
    N, dtype, P, m, env = c
    return f"N{N}-{C.dname(dtype)}-P{P}-m{m}-" + ",".join(f"{k[3:]}={v}" for k, v in env.items())


@pytest.mark.parametrize("case", SWITCH_CASES, ids=[switch_id(c) for c in SWITCH_CASES])
def test_switches(case, monkeypatch):
    """Six iterations on the copy transport, host path and check_every = 4, under one switch setting; the plan the
    model of pcg_cases gives for the setting is the one in the trace."""
    N, dtype, P, m, env = case
    set_env(monkeypatch, env)
    G, plan = PC.model(N, dtype, P, m, env)
    want = reference(N, dtype, PC.DECOMPOSED_ITERS, m)
    u, v, w = C.cg_velocity(N, dtype, PC.seed(N))
    with make(N, dtype, P=P) as fs:
        fs.set_pressure_preconditioner("jacobi", m)
        for every in (0, 4):
            fs.set_pressure_sync(every)
            check_solve(fs, u, v, w, TOL, PC.DECOMPOSED_ITERS, f"{switch_id(case)} [{plan}] sync={every}", want=want)
    check_plan(G, plan)


# ---- (e) -----------------------------------------------------------------------------------------------------------
VEL_N, VEL_TOL, VEL_MAX, VEL_STEPS = 40, 1e-2, 10, 2
VEL_NAMES = ("u", "v", "w")
VEL_CASES = [(9, 8, True), (6, 3, False)]  # (K, m, bound sources)
VEL_IDS = ["K9-jacobi8-bound", "K6-jacobi3-unbound"]
# the settings of the unpreconditioned step, the stored zero and the trapezoid
SETTINGS = CG_STEP_SETTINGS + [{"SF_ZERO_SKIP": "0"}, {"SF_TRAP": "5"}]
_VEL_REFERENCE = {}


def vel_reference(K, m):
    """Two vel_step composed in numpy; bound sources and sources uploaded again before every step are one input."""
    if (K, m) not in _VEL_REFERENCE:
        f = random_fields(VEL_N, np.float32, 41)
        g, outs = dict(f), []
        for _ in range(VEL_STEPS):
            out = reference_vel_step(g, K, VEL_TOL, VEL_MAX, m, sources={n: f[n] for n in ("u0", "v0", "w0")})
            outs.append(out)
            g = dict(f, u=out["u"], v=out["v"], w=out["w"])
        _VEL_REFERENCE[(K, m)] = outs
    return _VEL_REFERENCE[(K, m)]


def vel_steps_with_pcg(K, m, bound, P, every, outs, what):
    f = random_fields(VEL_N, np.float32, 41)
    with make(VEL_N, np.float32, K=K, P=P) as fs:
        upload_all(fs, f)
        if bound:
            for slot, n in (("user0", "u0"), ("user1", "v0"), ("user2", "w0")):
                fs.upload(slot, f[n])
            fs.bind_sources("user0", "user1", "user2", None)
        fs.set_pressure_solver("cg", VEL_TOL, VEL_MAX)
        fs.set_pressure_sync(every)
        fs.set_pressure_preconditioner("jacobi", m)
        for step, out in enumerate(outs):
            fs.vel_step()
            info = fs.pressure_info()
            print(f"{what} step {step}: {info}")
            assert (info["solver"], info["status"], info["iterations"]) == (S().SF_PRESSURE_CG, out["status"], out["iterations"])
            assert D.bits(info["rel_residual"]) == D.bits(out["rel_residual"])
            assert info["solves_total"] == 2 * (step + 1)
            for n in VEL_NAMES:
                assert_same_bits(fs.download(n), out[n], f"{what} step {step}: {n}")
            if not bound:
                for n in ("u0", "v0", "w0"):  # the sources of the next step
                    fs.upload(n, f[n])


@pytest.mark.parametrize("every", [0, 4], ids=["host", "sync4"])
@pytest.mark.parametrize("env", [{}] + SETTINGS, ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()) or "default")
@pytest.mark.parametrize("P", [1, 4], ids=["P1", "P4"])
@pytest.mark.parametrize("K,m,bound", VEL_CASES, ids=VEL_IDS)
def test_vel_step_with_the_preconditioner_under_switches(K, m, bound, P, env, every, monkeypatch):
    """Two vel_step at N = 40 fp32 with CG (1e-2, 10): under the default switches and under every setting the bits of
    the numpy composition, pressure_info after every step included. K = 9 with SF_MARCH_MINCELLS_K=0: the marching
    diffuse leaves a dead i-shell in front of project_cg and jacobi:8 is two marching passes. jacobi:3 is a pair and a
    single sweep (two passes: z ends in the buffer it started in) except under SF_FUSE2=0, and under SF_GHOST=1 at
    P = 4, where it is three single sweeps and every M leaves z in the other buffer of the ping-pong."""
    outs = vel_reference(K, m)
    assert all(o["iterations"] >= 1 for o in outs)
    set_env(monkeypatch, env)
    vel_steps_with_pcg(K, m, bound, P, every, outs, f"K={K} m={m} bound={bound} P={P} {env} sync={every}")


# ---- (f) -----------------------------------------------------------------------------------------------------------
FORCES = {"eps": 0.3, "beta": 0.5, "ambient": 0.1, "axis": 1}
_FULL_REFERENCE = {}


def full_reference(N, dtype, K, m, steps):
    """`steps` steps of vel_step + dens_step with MacCormack for both, confinement, buoyancy, bound velocity sources and
    CG with jacobi:m, composed from forces_ref, stable_ref, maccormack_ref and pressure_pcg_ref. Per step the fields
    and the second projection's outcome."""
    key = (N, C.dname(dtype), K, m, steps)
    if key not in _FULL_REFERENCE:
        f = random_fields(N, dtype, 47)
        T = np.dtype(dtype).type
        g, out = {n: a.copy() for n, a in f.items()}, []
        for _ in range(steps):
            o = reference_vel_step(g, K, VEL_TOL, VEL_MAX, m, sources={n: f[n] for n in ("u0", "v0", "w0")}, forces=FORCES,
                                   maccormack=True)
            for n in VEL_NAMES:
                g[n] = o[n]
            MC.dens_step(g["dens"], g["dens0"], g["u"], g["v"], g["w"], T(DIFF), T(DT), K, MC.MACCORMACK)
            out.append(({n: g[n].copy() for n in VEL_NAMES + ("dens",)}, o))
        _FULL_REFERENCE[key] = out
    return _FULL_REFERENCE[key]


@pytest.mark.parametrize("P", [1, 4], ids=["P1", "P4"])
def test_everything_on_at_once(P, monkeypatch):
    """op_add_forces, op_advect_mc and op_project_cg take a ScratchAlias over the same three buffers one after the
    other; z and its partner are the preconditioner's own and must come through. K = 9 with the marching kernel on."""
    N, dtype, K, m, steps = 40, np.float32, 9, 8, 2
    want = full_reference(N, dtype, K, m, steps)
    assert all(o["iterations"] >= 1 for _, o in want)
    set_env(monkeypatch, PC.MARCH)
    f = random_fields(N, dtype, 47)
    with make(N, dtype, K=K, P=P) as fs:
        upload_all(fs, f)
        for slot, n in (("user0", "u0"), ("user1", "v0"), ("user2", "w0")):
            fs.upload(slot, f[n])
        fs.bind_sources("user0", "user1", "user2", None)
        fs.set_vorticity_confinement(FORCES["eps"])
        fs.set_buoyancy(FORCES["beta"], FORCES["ambient"], FORCES["axis"])
        fs.set_advection(S().SF_ADVECT_MACCORMACK, S().SF_ADVECT_MACCORMACK)
        fs.set_pressure_solver("cg", VEL_TOL, VEL_MAX)
        fs.set_pressure_preconditioner("jacobi", m)
        for step, (fields, out) in enumerate(want):
            fs.vel_step()
            info = fs.pressure_info()
            fs.dens_step()
            print(f"P={P} step {step}: {info}")
            assert (info["solver"], info["status"], info["iterations"]) == (S().SF_PRESSURE_CG, out["status"], out["iterations"])
            assert D.bits(info["rel_residual"]) == D.bits(out["rel_residual"])
            for n, a in fields.items():
                assert_same_bits(fs.download(n), a, f"P={P} step {step}: {n}")


# ---- (g) -----------------------------------------------------------------------------------------------------------
GRAPH_TOL, GRAPH_MAX = 3e-2, 30  # both projections of the first CG step converge: 15 applications of M at jacobi:3, 7 at 6
# (id, switches, sweeps of the first and of the second CG step): an M of an odd number of passes leaves z and its partner
# swapped. jacobi:3 is `2Z 1`, two passes, wherever pairs are fused; with SF_FUSE2=0 it is three single sweeps. Under the
# default switches jacobi:6 is `2Z 2 2`.
GRAPH_CASES = [("FUSE2=0-jacobi3-jacobi8", {"SF_FUSE2": "0"}, 3, 8), ("jacobi6-jacobi8", {}, 6, 8)]


@pytest.mark.parametrize("name,env,m1,m2", GRAPH_CASES, ids=[c[0] for c in GRAPH_CASES])
def test_graphs_replay_around_uncaptured_preconditioned_steps(name, env, m1, m2, monkeypatch):
    """SF_GRAPH=1 on one slab (graphs are taken there only): Jacobi step, dens_step, CG step with jacobi:m1, dens_step,
    Jacobi step, CG step with jacobi:m2, Jacobi step on one context equal the same sequence without graphs. The first
    preconditioned solve allocates the two owning slots of z in the middle of the run, and every capture key after it
    contains them. pressure_info after every vel_step is the one of the run without graphs, the totals included: a
    replayed Jacobi step says what its capture noted of its two projections.

    The first CG step leaves z and its partner swapped: asserted from the trace, in which the passes that write z's two
    buffers during that step are odd in number (an odd number of passes per M, run an odd number of times in the two
    projections). The dens_step, the Jacobi step and the second CG step after it run on the swapped pair. What the
    second CG step leaves is printed, not asserted."""
    N, dtype = VEL_N, np.float32
    passes_per_M = len(PC.parse_plan(PC.model(N, dtype, 1, m1, env)[1]))
    assert passes_per_M % 2 == 1, (m1, env, passes_per_M)
    set_env(monkeypatch, env)
    f = random_fields(N, dtype, 43)
    sequence = (("jacobi", 0), None, ("cg", m1), None, ("jacobi", 0), ("cg", m2), ("jacobi", 0))
    trace = os.environ["SF_TRACE_SCHEDULE"].split(",")[0]
    out = []
    for graph in ("0", "1"):
        monkeypatch.setenv("SF_GRAPH", graph)
        with make(N, dtype, K=6) as fs:
            upload_all(fs, f)
            infos, cg_passes = [], []
            for item in sequence:
                if item is None:
                    fs.dens_step()
                    continue
                solver, m = item
                fs.set_pressure_solver(solver, GRAPH_TOL, GRAPH_MAX)
                if m:
                    fs.set_pressure_preconditioner("jacobi", m)
                    fs.sync()
                before = len(slab0_ops(trace))
                fs.vel_step()
                i = fs.pressure_info()
                infos.append((i["solver"], i["status"], i["iterations"], D.bits(i["rel_residual"]), i["solves_total"],
                              i["iterations_total"]))
                if m:
                    fs.sync()
                    count, zbufs, last = passes_of_M(slab0_ops(trace)[before:], cg_passes[0][1] if cg_passes else None)
                    print(f"SF_GRAPH={graph} jacobi:{m}: {count} passes of M wrote buffers {sorted(zbufs)}; z ends in {last}; {i}")
                    cg_passes.append((count, zbufs, last))
            fs.sync()
            out.append(({n: fs.download(n) for n in S().FIELD_NAMES}, infos))
        (count, zbufs, _), _ = cg_passes
        assert len(zbufs) == 2 and count % passes_per_M == 0 and count % 2 == 1, (name, graph, count, zbufs)
    assert out[0][1] == out[1][1]
    J, CG = S().SF_PRESSURE_JACOBI, S().SF_PRESSURE_CG
    assert [i[0] for i in out[0][1]] == [J, CG, J, CG, J]
    assert all(i[2] >= 1 for i in out[0][1] if i[0] == CG)
    for n in S().FIELD_NAMES:
        assert_same_bits(out[1][0][n], out[0][0][n], f"{n}: SF_GRAPH=1 against no graphs")


def test_a_replayed_step_reports_its_projections(monkeypatch):
    """SF_GRAPH=1, five Jacobi vel_step on one context: the slots' pointers come round again, so the later steps replay a
    cached graph. sf_pressure_info_get is the step's second projection after each of them, and solves_total and
    iterations_total count both projections of every step, replayed or captured."""
    monkeypatch.setenv("SF_GRAPH", "1")
    N, K = 16, 6
    f = random_fields(N, np.float32, 45)
    with make(N, np.float32, K=K) as fs:
        upload_all(fs, f)
        for step in range(5):
            fs.vel_step()
            i = fs.pressure_info()
            print(f"step {step}: {i}")
            assert (i["solver"], i["status"], i["iterations"], i["rel_residual"]) == (S().SF_PRESSURE_JACOBI, R.MAX_ITERS, K, -1.0)
            assert (i["solves_total"], i["iterations_total"]) == (2 * (step + 1), 2 * K * (step + 1))
