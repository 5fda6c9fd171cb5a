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

--moving adds the rows of SPEC §19 from a context of its own: the §17 step and the §19 step (a constant solid
velocity, sf_set_obstacle_velocity) after --warmup steps each; the single operators on a velocity component (b = 1, one
field) with the velocity unset (the masked kernels) and set (the moving ones): sf_diffuse_masked per sweep,
sf_advect_masked, and sf_project_cg ended after one iteration, whose difference is the cost of the two project halves
together (they have no entry point of their own); and the §19 step with sf_set_obstacles and sf_set_obstacle_velocity
called again before every step from slots already on the device, which is what a moving mask costs beyond its upload:
two synchronisations, the face codes, three field copies and the dropped graph cache.

  python tools/obstacle_step_bench.py --cases 256:f32 256:f64 [--maccormack] [--moving]
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


def moving_case(N, dtype, a):
    """The rows of --moving (SPEC §19)."""
    fs = context(N, dtype)
    fs.set_pressure_solver("cg", a.tol, a.max_iters)
    fs.set_pressure_sync(a.sync)
    fs.set_pressure_multigrid(*parse_mg(a.mg))
    fs.set_obstacle_multigrid(True)
    # the mask stays on the device in user3, so the density source of this context is not bound (dens0 is the source)
    fs.bind_sources("user0", "user1", "user2", None)
    fs.upload("user3", obstacle_mask(N, dtype, ["centred"]))
    fs.set_obstacles("user3")
    fs.set_obstacle_transport(True)
    vel = (0.05, -0.02, 0.03)  # domain units per unit time: dt N V = 1.28 cells per step along i at N = 256

    def velocity(on):
        if not on:
            fs.set_obstacle_velocity(None, None, None)
            return
        for slot, v in zip(("u0", "v0", "w0"), vel):
            fs.fill(slot, v)
        fs.set_obstacle_velocity("u0", "v0", "w0")

    def step_again():
        fs.set_obstacles("user3")
        for slot, v in zip(("u0", "v0", "w0"), vel):
            fs.fill(slot, v)
        fs.set_obstacle_velocity("u0", "v0", "w0")
        fs.vel_step()
        fs.dens_step()

    def step():
        fs.vel_step()
        fs.dens_step()

    rows = []
    for on in (False, True):
        velocity(on)
        for _ in range(a.warmup):
            step()
        fs.sync()
        i0 = fs.pressure_info()["iterations_total"]
        v = best_of(fs, a.reps, a.steps, fs.vel_step)
        its = (fs.pressure_info()["iterations_total"] - i0) / (2.0 * a.steps * a.reps)
        d = best_of(fs, a.reps, a.steps, fs.dens_step)
        rows.append({"case": "moving_step", "grid": N, "dtype": dtype, "solid_velocity": on, "vel_step_ms": round(v, 4),
                     "dens_step_ms": round(d, 4), "step_ms": round(v + d, 4), "iterations_per_projection": round(its, 2),
                     "last_status": fs.pressure_info()["status"]})
    whole = best_of(fs, a.reps, a.steps, step)
    again = best_of(fs, a.reps, a.steps, step_again)
    rows.append({"case": "moving_reset", "grid": N, "dtype": dtype, "step_ms": round(whole, 4),
                 "step_with_mask_and_velocity_set_again_ms": round(again, 4), "extra_ms": round(again - whole, 4)})
    # the single operators on one velocity component; dens and dens0 are scratch here
    ops = {"diffuse_b1": lambda: fs.diffuse_masked(1, "dens0", "u", DIFF),
           "advect_b1": lambda: fs.advect_masked(1, "dens0", "u", "u", "v", "w"),
           "project_cg_1": lambda: (fs.copy_field("dens", "u"), fs.project_cg("dens", "v", "w", "u0", "v0", 1e-30, 1)),
           "copy_field": lambda: fs.copy_field("dens", "u")}
    took = {}
    for on in (False, True):
        velocity(on)
        for name, call in ops.items():
            call()
            took[name, on] = best_of(fs, a.reps, 10, call)
    for name in ("diffuse_b1", "advect_b1", "project_cg_1"):
        m, v = took[name, False], took[name, True]
        if name == "project_cg_1":  # without the copy that restores u
            m, v = m - took["copy_field", False], v - took["copy_field", True]
        row = {"case": "moving_operator", "grid": N, "dtype": dtype, "op": name, "masked_ms": round(m, 5), "moving_ms": round(v, 5),
               "ratio": round(v / m, 3)}
        if name == "diffuse_b1":
            row.update(sweeps=K, masked_ms_per_sweep=round(m / K, 5), moving_ms_per_sweep=round(v / K, 5))
        if name == "project_cg_1":
            row["halves_extra_ms"] = round(v - m, 5)
        rows.append(row)
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
    ap.add_argument("--moving", action="store_true", help="add the steps and the operators of SPEC §19")
    ap.add_argument("--only-moving", action="store_true", help="the rows of --moving alone")
    a = ap.parse_args()
    for c in a.cases:
        n, t = c.split(":")
        if not a.only_moving:
            for row in limited(a.limit, lambda: case(int(n), t, a)):
                print(json.dumps(row), flush=True)
        if a.moving or a.only_moving:
            for row in limited(a.limit, lambda: moving_case(int(n), t, a)):
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
