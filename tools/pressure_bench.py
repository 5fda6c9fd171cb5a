#!/usr/bin/env python3
"""Time the conjugate-gradient projection of docs/SPEC.md §11 (measurement aid, not the benchmark).

SPEC §5 inputs with bound sources (the benchmark's workload), K = 20, one process, one context per case. Every case runs
under its own time limit (--limit seconds, SIGALRM: the process ends with status 124 and starts nothing more).

  iteration   sf_project_cg with a tolerance nothing reaches, max_iters = M and max_iters = 0, host wall time from the
              call to its return (the solve synchronises): (t_M - t_0) / iterations is one iteration, host
              synchronisations included. Its compulsory traffic is 11 words per cell (apply: d in, q out; update: p, d,
              r, q in, p, r out; direction: r, d in, d out); `ceiling_share` = the time those bytes take at the
              sf_measure_copy_bandwidth of the same run / the measured time. Kernel times: run one case under
              rocprofv3 --kernel-trace --stats; measured time - kernel time is the host's share.
  sync        the same (t_M - t_0) / iterations on one context per grid and decomposition (one slab, and --sync-slabs
              logical slabs with the device-local copy transport), for every check_every of --check-every (sf_set_pressure_sync;
              "max" = max_iters: one host wait per solve; 0 = the host path, the yardstick) one after another in one
              process, so that the variants see the same machine. The clock stops after sf_sync, so both paths are
              timed to the end of the gradient subtraction on every slab. host_waits is that of the M-iteration solve.
  precond     (--precond 0,2,4,8) one context per grid; for every sweep count M of the Jacobi preconditioner of SPEC §11.2
              (0: none): the time of one iteration as in `sync` (with --sync M' the scalars on the device, read every M'
              iterations; without, on the host), the iterations to tol = 1e-3 from the same state and the time of that
              projection, and, for --step-case, the step with CG at each --tols. --mg NU[:LEVELS[:COARSE]],... adds the
              multigrid V-cycle of SPEC §11.3 at each of those settings to the same table (rows with "mg"), measured
              on the same context, after the sweep counts. With --obstacle the masked runs take those settings too
              (sf_set_obstacle_multigrid, SPEC §16), and every "mg" row carries vcycle_ms: one z = M(r) alone
              (sf_precondition, or sf_precondition_masked under the mask), the best of --reps batches of ten.
  step        vel_step + dens_step per step (host wall time of --steps steps between syncs) with Jacobi K = 20 and with
              CG at each --tols, the iterations per step, and sf_poisson_residual / max_div of what the last step left.

  python tools/pressure_bench.py                       # iteration: 256^3 fp32, 512^3 fp32, 512^3 fp64; step: 256^3 fp32
  python tools/pressure_bench.py --cases 256:f32 --no-step   # e.g. under rocprofv3 --kernel-trace --stats
  python tools/pressure_bench.py --sync --cases 64:f32 128:f32 256:f32 512:f32 256:f64   # where the scalars live
  python tools/pressure_bench.py --precond 0,2,4,8 --sync 8 --cases 64:f32 128:f32 256:f32 512:f32 256:f64
  python tools/pressure_bench.py --precond 0,8 --mg 2,2:0:16,1,2:4 --cases 64:f32 128:f32 256:f32 512:f32 256:f64
  python tools/pressure_bench.py --precond 8 --mg 2:0:8,2:4:8 --obstacle centred --sync 8 --no-step --cases 256:f32 256:f64 512:f32
"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, DIFF, VISC, K = 0.1, 1e-4, 1e-4, 20
WORDS_PER_ITERATION = 11


def context(N, dtype, slabs=1):
    from bench import upload_inputs
    from fluidsolvergpu_amd import solver as S

    fs = S.FluidSolver(N, dtype=dtype, iters=K, dt=DT, diff=DIFF, visc=VISC, nslabs_local=slabs)
    upload_inputs(fs, N, DT)
    fs.bind_sources()
    return fs


def iteration_case(N, dtype, iters, reps):
    fs = context(N, dtype)
    for _ in range(2):
        fs.vel_step()
        fs.dens_step()
    fs.sync()
    state = {n: fs.download(n) for n in ("u", "v", "w")}

    def solve(max_iters):
        for n, a in state.items():
            fs.upload(n, a)
        fs.sync()
        t0 = time.perf_counter()
        info = fs.project_cg("u", "v", "w", "u0", "v0", 1e-30, max_iters)
        return (time.perf_counter() - t0) * 1e3, info

    solve(2)
    t0 = min(solve(0)[0] for _ in range(reps))
    runs = [solve(iters) for _ in range(reps)]
    tm, info = min(runs, key=lambda r: r[0])
    gbps = fs.copy_bandwidth_gbps(1 << 30, 5)
    fs.close()
    per = (tm - t0) / max(info["iterations"], 1)
    compulsory = WORDS_PER_ITERATION * float(N) ** 3 * (4 if dtype == "f32" else 8) / (gbps * 1e9) * 1e3
    return {"case": "iteration", "grid": N, "dtype": dtype, "iterations": info["iterations"], "status": info["status"],
            "solve_ms": round(tm, 4), "solve_0_iterations_ms": round(t0, 4), "iteration_ms": round(per, 4),
            "copy_gbps": round(gbps, 1), "iteration_compulsory_ms": round(compulsory, 4),
            "ceiling_share_incl_host": round(compulsory / per, 3)}


def sync_case(N, dtype, slabs, iters, reps, check_every):
    """One row per check_every: the time of one iteration with the scalars on the host (0) or on the device."""
    fs = context(N, dtype, slabs)
    for _ in range(2):
        fs.vel_step()
        fs.dens_step()
    fs.sync()
    state = {n: fs.download(n) for n in ("u", "v", "w")}

    def solve(max_iters):
        for n, a in state.items():
            fs.upload(n, a)
        fs.sync()
        t0 = time.perf_counter()
        info = fs.project_cg("u", "v", "w", "u0", "v0", 1e-30, max_iters)
        fs.sync()  # the device path returns with the closing set_bnd, the gradient and other slabs' work in flight
        return (time.perf_counter() - t0) * 1e3, info, fs.pressure_sync["host_waits"]

    rows = []
    for m in check_every:
        fs.set_pressure_sync(iters if m == "max" else int(m))
        solve(2)
        t0 = min(solve(0)[0] for _ in range(reps))
        tm, info, waits = min((solve(iters) for _ in range(reps)), key=lambda r: r[0])
        rows.append({"case": "sync", "grid": N, "dtype": dtype, "slabs": slabs, "check_every": m,
                     "iterations": info["iterations"], "status": info["status"], "host_waits": waits,
                     "solve_ms": round(tm, 4), "solve_0_iterations_ms": round(t0, 4),
                     "iteration_ms": round((tm - t0) / max(info["iterations"], 1), 5)})
    base = rows[0]["iteration_ms"]
    for r in rows:
        r["vs_first"] = round(r["iteration_ms"] / base, 3) if base > 0 else None
    fs.close()
    return rows


def parse_mg(spec):
    """NU[:LEVELS[:COARSE]] -> (nu, max_levels, coarse_sweeps), the driver's --pressure-mg."""
    parts = [int(x) for x in spec.split(":")]
    if not 1 <= len(parts) <= 3 or parts[0] < 1:
        raise SystemExit(f"--mg takes NU[:LEVELS[:COARSE]] with NU >= 1, not {spec}")
    return tuple(parts + [0, 8][len(parts) - 1:])


def set_precond(fs, sweeps):
    """sweeps: a count of Jacobi sweeps (0: none) or the (nu, max_levels, coarse_sweeps) of the V-cycle."""
    if isinstance(sweeps, tuple):
        fs.set_pressure_multigrid(*sweeps)
        return
    fs.set_pressure_multigrid(0)
    if sweeps > 0:
        fs.set_pressure_preconditioner("jacobi", sweeps)
    else:
        fs.set_pressure_preconditioner("none")


def precond_label(sweeps):
    return {"sweeps": None, "mg": "%d:%d:%d" % sweeps} if isinstance(sweeps, tuple) else {"sweeps": sweeps}


def obstacle_mask(N, dtype, specs):
    """The mask of the driver's --obstacle values (docs/SPEC.md §15), and `centred`: the box of the cells i with
    0.3 N < i <= 0.6 N per axis. (N+2)^3, [k, j, i], 1 in solid cells."""
    import numpy as np

    k, j, i = np.meshgrid(*(np.arange(N + 2, dtype=np.float64),) * 3, indexing="ij", sparse=True)
    solid = np.zeros((N + 2,) * 3, bool)
    for spec in specs:
        if spec == "centred":
            spec = "box:%d,%d,%d:%d,%d,%d" % ((int(0.3 * N) + 1,) * 3 + (int(0.6 * N),) * 3)
        kind, a, b = spec.split(":")
        a = [float(x) for x in a.split(",")]
        if kind == "box":
            b = [float(x) for x in b.split(",")]
            solid |= (i >= a[0]) & (i <= b[0]) & (j >= a[1]) & (j <= b[1]) & (k >= a[2]) & (k <= b[2])
        elif kind == "sphere":
            solid |= ((i - a[0]) ** 2 + (j - a[1]) ** 2) + (k - a[2]) ** 2 <= float(b) ** 2
        else:
            raise SystemExit(f"--obstacle takes centred, box:I0,J0,K0:I1,J1,K1 or sphere:CX,CY,CZ:R, not {spec}")
    solid[0], solid[-1], solid[:, 0], solid[:, -1], solid[:, :, 0], solid[:, :, -1] = (False,) * 6
    return solid.astype(np.float32 if dtype == "f32" else np.float64)


def precond_case(N, dtype, iters, reps, sweeps, check_every, max_iters, obstacle=None):
    """One row per sweep count: an iteration's time, and the projection to tol = 1e-3 from the same state. obstacle: the
    --obstacle values; the solves then run under that mask (sf_set_obstacles) and the rows say how many cells are fluid."""
    fs = context(N, dtype)
    for _ in range(2):
        fs.vel_step()
        fs.dens_step()
    fs.sync()
    state = {n: fs.download(n) for n in ("u", "v", "w")}
    fs.set_pressure_sync(check_every)
    if obstacle:
        fs.set_obstacles(obstacle_mask(N, dtype, obstacle), slot="dens0")
        fs.set_obstacle_multigrid(True)  # (the V-cycle rows run the masked cycle of SPEC §16)

    def vcycle_ms():
        """One z = M(r) alone, between syncs: ten in a row, the best batch."""
        apply = fs.precondition_masked if obstacle else fs.precondition
        fs.upload("v0", state["u"])  # (any right-hand side: the cycle's time does not depend on it)
        apply("u0", "v0")
        best = 1e30
        for _ in range(reps):
            fs.sync()
            t0 = time.perf_counter()
            for _ in range(10):
                apply("u0", "v0")
            fs.sync()
            best = min(best, (time.perf_counter() - t0) * 1e2)
        return round(best, 5)

    def solve(tol, limit):
        for n, a in state.items():
            fs.upload(n, a)
        fs.sync()
        t0 = time.perf_counter()
        info = fs.project_cg("u", "v", "w", "u0", "v0", tol, limit)
        fs.sync()
        return (time.perf_counter() - t0) * 1e3, info

    rows = []
    for m in sweeps:
        set_precond(fs, m)
        solve(1e-30, 2)
        t0 = min(solve(1e-30, 0)[0] for _ in range(reps))
        tm, info = min((solve(1e-30, iters) for _ in range(reps)), key=lambda r: r[0])
        tp, done = min((solve(1e-3, max_iters) for _ in range(reps)), key=lambda r: r[0])
        rows.append({"case": "precond", "grid": N, "dtype": dtype, **precond_label(m), "check_every": check_every,
                     "obstacle": obstacle, "fluid_cells": fs.obstacles()["fluid_cells"],
                     "iteration_ms": round((tm - t0) / max(info["iterations"], 1), 5),
                     "iterations_1e-3": done["iterations"], "status_1e-3": done["status"],
                     "rel_residual": done["rel_residual"], "poisson_residual": fs.poisson_residual("u0", "v0"),
                     "projection_ms": round(tp, 4)})
        if isinstance(m, tuple):
            rows[-1]["vcycle_ms"] = vcycle_ms()
    fs.close()
    return rows


def step_case(N, dtype, steps, tols, max_iters, precond=0, check_every=0):
    out = []
    for tol in [None] + tols:
        if tol is None and precond != 0:
            continue  # (the Jacobi step has no preconditioner: timed once, with precond = 0)
        fs = context(N, dtype)
        if tol is not None:
            fs.set_pressure_solver("cg", tol, max_iters)
            fs.set_pressure_sync(check_every)
            set_precond(fs, precond)
        for _ in range(3):
            fs.vel_step()
            fs.dens_step()
        best, its = 1e30, 0
        for _ in range(3):
            fs.sync()
            i0 = fs.pressure_info()["iterations_total"]
            t0 = time.perf_counter()
            for _ in range(steps):
                fs.vel_step()
                fs.dens_step()
            fs.sync()
            best = min(best, (time.perf_counter() - t0) * 1e3 / steps)
            its = (fs.pressure_info()["iterations_total"] - i0) / (2.0 * steps)
        info = fs.pressure_info()
        out.append({"case": "step", "grid": N, "dtype": dtype, "solver": "jacobi" if tol is None else "cg", "tol": tol,
                    "precond_sweeps": precond if not isinstance(precond, tuple) else None,
                    "mg": "%d:%d:%d" % precond if isinstance(precond, tuple) else None, "check_every": check_every,
                    "step_ms": round(best, 4), "iterations_per_projection": round(its, 2), "last_status": info["status"],
                    "last_rel_residual": info["rel_residual"], "poisson_residual": fs.poisson_residual("u0", "v0"),
                    "max_div": fs.diagnostics()["max_div"]})
        fs.close()
    return out


def limited(seconds, call):
    def expired(*_):
        print(json.dumps({"error": f"case exceeded its {seconds} s limit"}), flush=True)
        os._exit(124)

    signal.signal(signal.SIGALRM, expired)
    signal.alarm(seconds)
    try:
        return call()
    finally:
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["256:f32", "512:f32", "512:f64"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step-case", default="256:f32")
    ap.add_argument("--tols", nargs="+", type=float, default=[1e-2, 1e-3])
    ap.add_argument("--max-iters", type=int, default=200)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--sync", nargs="?", const=True, default=False,
                    help="alone: only the sync cases; with --precond: --sync M keeps the scalars on the device")
    ap.add_argument("--precond", default=None, help="comma-separated sweep counts, e.g. 0,2,4,8: only the precond cases")
    ap.add_argument("--mg", default=None, help="comma-separated V-cycle settings NU[:LEVELS[:COARSE]] (SPEC §11.3), e.g. "
                    "2,2:0:16,1,2:4: added to the precond cases (alone: --precond 0)")
    ap.add_argument("--obstacle", action="append", default=None,
                    help="with --precond: solve under this mask too (centred, box:I0,J0,K0:I1,J1,K1, sphere:CX,CY,CZ:R; may "
                         "be repeated): every case runs without and with it")
    ap.add_argument("--check-every", nargs="+", default=["0", "1", "8", "max"])
    ap.add_argument("--sync-slabs", type=int, default=4)
    a = ap.parse_args()
    if a.precond is not None or a.mg is not None:
        sweeps = [int(m) for m in (a.precond or "0").split(",")]
        sweeps += [parse_mg(x) for x in a.mg.split(",")] if a.mg else []
        every = 0 if a.sync in (False, True) else int(a.sync)
        for c in a.cases:
            n, t = c.split(":")
            for ob in ([None, a.obstacle] if a.obstacle else [None]):
                for row in limited(a.limit, lambda: precond_case(int(n), t, a.iters, a.reps, sweeps, every, a.max_iters, ob)):
                    print(json.dumps(row), flush=True)
        if not a.no_step:
            n, t = a.step_case.split(":")
            for m in sweeps:
                for row in limited(3 * a.limit, lambda: step_case(int(n), t, a.steps, a.tols, a.max_iters, m, every)):
                    print(json.dumps(row), flush=True)
        return
    if a.sync:
        for c in a.cases:
            n, t = c.split(":")
            for slabs in (1, a.sync_slabs):
                for row in limited(a.limit, lambda: sync_case(int(n), t, slabs, a.iters, a.reps, a.check_every)):
                    print(json.dumps(row), flush=True)
        return
    for c in a.cases:
        n, t = c.split(":")
        print(json.dumps(limited(a.limit, lambda: iteration_case(int(n), t, a.iters, a.reps))), flush=True)
    if not a.no_step:
        n, t = a.step_case.split(":")
        for row in limited(3 * a.limit, lambda: step_case(int(n), t, a.steps, a.tols, a.max_iters)):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
