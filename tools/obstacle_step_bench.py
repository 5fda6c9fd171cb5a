#!/usr/bin/env python3
"""Time the steps and the single operators of mask-aware transport, docs/SPEC.md §17 (measurement aid, not the benchmark).

SPEC §5 inputs with bound sources (the benchmark's workload), K = 20, one process, one context per case, the centred box
of tools/pressure_bench.py as the obstacle, CG to --tol with the masked V-cycle --mg (SPEC §16) and the scalars on the
device (--sync). Every case runs under its own time limit (--limit seconds, SIGALRM: the process ends with status 124
and starts nothing more). After --warmup steps, with sf_set_obstacle_transport off (the step of §15, the yardstick) and on:

  step        host wall time of --steps vel_step between syncs, and of --steps dens_step, per step, best of --reps; the
              CG iterations per projection.
  operators   sf_diffuse / sf_diffuse_masked (K sweeps: ms per sweep) and sf_advect / sf_advect_masked on the density,
              ten calls between syncs, best of --reps.

--maccormack adds the column of SPEC §18: a third step row with the setting on, both schemes SF_ADVECT_MACCORMACK and
sf_set_obstacle_maccormack(1), and the operators sf_advect_maccormack / sf_advect_maccormack_masked next to the four
above, with the cost of each second pass alone (the operator minus its first pass) and their ratio.

  python tools/obstacle_step_bench.py --cases 256:f32 256:f64 [--maccormack]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pressure_bench import DIFF, K, context, limited, obstacle_mask, parse_mg  # noqa: E402


def best_of(fs, reps, n, call):
    """ms per call: n calls between syncs, the best of reps batches."""
    best = 1e30
    for _ in range(reps):
        fs.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        fs.sync()
        best = min(best, (time.perf_counter() - t0) * 1e3 / n)
    return best


def case(N, dtype, a):
    fs = context(N, dtype)
    fs.set_pressure_solver("cg", a.tol, a.max_iters)
    fs.set_pressure_sync(a.sync)
    fs.set_pressure_multigrid(*parse_mg(a.mg))
    fs.set_obstacle_multigrid(True)
    fs.set_obstacles(obstacle_mask(N, dtype, ["centred"]), slot="dens0")
    rows = []
    for on, mc in ((False, False), (True, False)) + (((True, True),) if a.maccormack else ()):
        fs.set_obstacle_transport(on)
        if a.maccormack:
            fs.set_obstacle_maccormack(mc)
            fs.set_advection(1 if mc else 0, 1 if mc else 0)
        for _ in range(a.warmup):
            fs.vel_step()
            fs.dens_step()
        fs.sync()
        i0 = fs.pressure_info()["iterations_total"]
        vel = best_of(fs, a.reps, a.steps, fs.vel_step)
        its = (fs.pressure_info()["iterations_total"] - i0) / (2.0 * a.steps * a.reps)
        dens = best_of(fs, a.reps, a.steps, fs.dens_step)
        rows.append({"case": "step", "grid": N, "dtype": dtype, "obstacle_transport": on, "obstacle_maccormack": mc, "mg": a.mg, "tol": a.tol,
                     "vel_step_ms": round(vel, 4), "dens_step_ms": round(dens, 4), "step_ms": round(vel + dens, 4),
                     "iterations_per_projection": round(its, 2), "last_status": fs.pressure_info()["status"]})
    # the single operators on the density (one field): u0 and v0 are scratch between steps
    fs.vel_step()
    fs.sync()
    ops = {"diffuse": lambda: fs.diffuse(0, "u0", "dens", DIFF),
           "diffuse_masked": lambda: fs.diffuse_masked(0, "u0", "dens", DIFF),
           "advect": lambda: fs.advect(0, "v0", "dens", "u", "v", "w"),
           "advect_masked": lambda: fs.advect_masked(0, "v0", "dens", "u", "v", "w")}
    if a.maccormack:
        fs.set_advection(0, 0)
        ops["advect_maccormack"] = lambda: fs.advect_maccormack(0, "v0", "dens", "u", "v", "w")
        ops["advect_maccormack_masked"] = lambda: fs.advect_maccormack_masked(0, "v0", "dens", "u", "v", "w")
    took = {}
    for name, call in ops.items():
        call()
        ms = best_of(fs, a.reps, 10, call)
        took[name] = ms
        row = {"case": "operator", "grid": N, "dtype": dtype, "op": name, "ms": round(ms, 5)}
        if name.startswith("diffuse"):
            row["sweeps"] = K
            row["ms_per_sweep"] = round(ms / K, 5)
        rows.append(row)
    if a.maccormack:
        p2, p2m = took["advect_maccormack"] - took["advect"], took["advect_maccormack_masked"] - took["advect_masked"]
        rows.append({"case": "second_pass", "grid": N, "dtype": dtype, "advect_mc_ms": round(p2, 5),
                     "advect_mc_masked_ms": round(p2m, 5), "ratio": round(p2m / p2, 3),
                     "operator_ratio": round(took["advect_maccormack_masked"] / took["advect_maccormack"], 3)})
    gbps = fs.copy_bandwidth_gbps(1 << 30, 5)
    word = 4 if dtype == "f32" else 8
    rows.append({"case": "bytes", "grid": N, "dtype": dtype, "copy_gbps": round(gbps, 1),
                 "masked_sweep_4_words_ms": round(4 * float(N) ** 3 * word / (gbps * 1e9) * 1e3, 5)})
    fs.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["256:f32", "256:f64"])
    ap.add_argument("--mg", default="2:0:8")
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--max-iters", type=int, default=200)
    ap.add_argument("--sync", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150)
    ap.add_argument("--maccormack", action="store_true", help="add the step and the operators of SPEC §18")
    a = ap.parse_args()
    for c in a.cases:
        n, t = c.split(":")
        for row in limited(a.limit, lambda: case(int(n), t, a)):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
