#!/usr/bin/env python3
"""Time the reductions and diagnostics of docs/SPEC.md §10 (measurement aid, not the benchmark).

SPEC §5 inputs with bound sources (the benchmark's workload), K = 20. Both calls synchronise and hand their result to
the host, so what a caller pays is host wall time from the call to its return on an idle context: that is what is
timed (min and median over --reps calls). Per case, in one process:
  diagnostics_ms       sf_diagnostics_get: u, v, w, dens read once (4 words per cell compulsory)
  reduce_sum_ms        one sf_reduce(SF_RED_SUM) (1 word per cell)
  copy_gbps            sf_measure_copy_bandwidth of the same run (1 GiB), and the time the compulsory bytes take at it
  *_of_ceiling         compulsory time / measured time
  step_ms              vel_step + dens_step per step, host wall time of --steps steps after a sync, monitoring off
  monitor1 / monitor10 the same loop with sf_diagnostics_get after every step / every 10th step, and its share of step_ms

  python tools/diagnostics_bench.py                          # 256^3 fp32, 512^3 fp32, 512^3 fp64
  python tools/diagnostics_bench.py --cases 256:f32 --reps 5 # one case (e.g. under rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, DIFF, VISC, K = 0.1, 1e-4, 1e-4, 20


def compulsory_ms(N, dtype, words, gbps):
    return words * float(N) ** 3 * (4 if dtype == "f32" else 8) / (gbps * 1e9) * 1e3


def wall(fs, call, reps, warmup=2):
    t = []
    for r in range(warmup + reps):
        fs.sync()
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    t = t[warmup:]
    return min(t), float(np.median(t))


def loop_ms(fs, steps, every):
    fs.sync()
    t0 = time.perf_counter()
    for s in range(steps):
        fs.vel_step()
        fs.dens_step()
        if every and s % every == 0:
            fs.diagnostics()
    fs.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def time_case(N, dtype, reps, steps):
    from bench import upload_inputs
    from fluidsolvergpu_amd import solver as S

    fs = S.FluidSolver(N, dtype=dtype, iters=K, dt=DT, diff=DIFF, visc=VISC)
    upload_inputs(fs, N, DT)
    fs.bind_sources()
    for _ in range(3):
        fs.vel_step()
        fs.dens_step()
    d_min, d_med = wall(fs, fs.diagnostics, reps)
    r_min, r_med = wall(fs, lambda: fs.reduce("sum", "dens"), reps)
    # best of three passes per variant, the variants interleaved
    loops = {0: [], 1: [], 10: []}
    for _ in range(3):
        for every in loops:
            loops[every].append(loop_ms(fs, steps, every))
    step, m1, m10 = (min(loops[e]) for e in (0, 1, 10))
    state = fs.diagnostics()
    fs.sync()
    gbps = fs.copy_bandwidth_gbps(1 << 30, 5)
    fs.close()
    c4, c1 = compulsory_ms(N, dtype, 4, gbps), compulsory_ms(N, dtype, 1, gbps)
    return {"grid": N, "dtype": dtype, "K": K, "reps": reps, "steps": steps, "copy_gbps": round(gbps, 1),
            "diagnostics_ms_min": round(d_min, 4), "diagnostics_ms_median": round(d_med, 4),
            "diagnostics_compulsory_ms": round(c4, 4), "diagnostics_of_ceiling": round(c4 / d_min, 3),
            "reduce_sum_ms_min": round(r_min, 4), "reduce_sum_ms_median": round(r_med, 4),
            "reduce_sum_compulsory_ms": round(c1, 4), "reduce_sum_of_ceiling": round(c1 / r_min, 3),
            "step_ms": round(step, 4), "monitor1_step_ms": round(m1, 4), "monitor10_step_ms": round(m10, 4),
            "monitor1_share": round((m1 - step) / step, 4), "monitor10_share": round((m10 - step) / step, 4),
            "nonfinite": state["nonfinite"], "cfl": state["cfl"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["256:f32", "512:f32", "512:f64"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    for c in a.cases:
        n, t = c.split(":")
        print(json.dumps(time_case(int(n), t, a.reps, a.steps)), flush=True)


if __name__ == "__main__":
    main()
