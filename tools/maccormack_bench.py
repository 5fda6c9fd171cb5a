#!/usr/bin/env python3
"""Time MacCormack advection (docs/SPEC.md §9) against the first-order advect it is built from (measurement aid, not
the benchmark).

SPEC §5 inputs with bound sources (the benchmark's workload), K = 20, two steps run first so that w is not zero. The
variants alternate call by call in one process; per variant the device-timer min and median over --reps calls after
--warmup.
  operators   sf_advect against sf_advect_maccormack (pass 1 into the scratch buffer, its exchange, pass 2), for one
              field (u into the u0 slot, b = 1) and for the three velocity components (three calls, b = 1, 2, 3, into
              the three x0 slots). Target: MacCormack <= 3.5 x the same-run sf_advect time (gathers: 8 against 8 + 16
              per field, plus hat's extra stream and the selects).
  step        vel_step + dens_step with the schemes off / on the velocity / on both.
  --forms     the one-field operators under SF_ADVECT_ROW = 0 (gather form), 2 (one cell per lane, neighbour-lane
              sharing) and 3 (one cell per lane, own pair loads), one context each.
Words per interior cell: advect 6 for the velocity components (their own velocity), 5 for the density; pass 2 adds the
velocity, d0 and hat read and d written: + 9 / + 6.

  python tools/maccormack_bench.py                               # 256^3 fp32, 512^3 fp32, 256^3 fp64
  python tools/maccormack_bench.py --cases 256:f32 --reps 5      # one case (e.g. under rocprofv3 --kernel-trace --stats)
  python tools/maccormack_bench.py --stats kernel_stats.csv      # the advect kernels of that run's trace
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, DIFF, VISC, K = 0.1, 1e-4, 1e-4, 20
STEP_VARIANTS = {"off": (0, 0), "vel": (1, 0), "both": (1, 1)}


def parse_cases(cases):
    return [(int(c.split(":")[0]), c.split(":")[1]) for c in cases]


def context(N, dtype):
    from bench import analytic_planes
    from fluidsolvergpu_amd import solver as S

    a = analytic_planes(N, 0, N + 2, DT, np.float32 if dtype == "f32" else np.float64)
    fs = S.FluidSolver(N, dtype=dtype, iters=K, dt=DT, diff=DIFF, visc=VISC)
    for n in ("u", "v", "w", "dens"):
        fs.upload(n, a[n])
    for b, n in ((1, "u"), (2, "v"), (3, "w"), (0, "dens")):
        fs.set_bnd(b, n)
    for slot, n in (("user0", "su"), ("user1", "sv"), ("user2", "sw"), ("user3", "sd")):
        fs.upload(slot, a[n])
    fs.bind_sources()
    for _ in range(2):
        fs.vel_step()
        fs.dens_step()
    fs.sync()
    return fs


def stats(t):
    return round(min(t) * 1e3, 1), round(float(np.median(t)) * 1e3, 1)


def timed(fs, call):
    fs.sync()
    fs.timer_start()
    call()
    return fs.timer_stop()


def time_operators(fs, reps, warmup, three=True):
    """us (min, median) of sf_advect / sf_advect_maccormack: one field, and the three velocity components. The outputs
    go to the x0 slots, which the bound-source steps do not read."""
    comps = (("u0", 1, "u"), ("v0", 2, "v"), ("w0", 3, "w"))
    ops = {"advect": fs.advect, "maccormack": fs.advect_maccormack}
    sets = {"one": comps[:1]}
    if three:
        sets["three"] = comps
    times = {(o, s): [] for o in ops for s in sets}
    for r in range(warmup + reps):
        for s, cs in sets.items():
            for o, fn in ops.items():
                ms = timed(fs, lambda: [fn(b, d, d0, "u", "v", "w") for d, b, d0 in cs])
                if r >= warmup:
                    times[(o, s)].append(ms)
    row = {}
    for s in sets:
        for o in ops:
            row[f"{o}_{s}_us_min"], row[f"{o}_{s}_us_median"] = stats(times[(o, s)])
        row[f"ratio_{s}_min"] = round(row[f"maccormack_{s}_us_min"] / row[f"advect_{s}_us_min"], 2)
        row[f"ratio_{s}_median"] = round(row[f"maccormack_{s}_us_median"] / row[f"advect_{s}_us_median"], 2)
    return row


def time_steps(fs, reps, warmup):
    times = {v: [] for v in STEP_VARIANTS}
    for r in range(warmup + reps):
        for v, schemes in STEP_VARIANTS.items():
            fs.set_advection(*schemes)
            ms = timed(fs, lambda: (fs.vel_step(), fs.dens_step()))
            if r >= warmup:
                times[v].append(ms)
    fs.set_advection(0, 0)
    row = {}
    for v, t in times.items():
        row[f"step_{v}_ms_min"] = round(min(t), 4)
        row[f"step_{v}_ms_median"] = round(float(np.median(t)), 4)
    for v in ("vel", "both"):
        row[f"step_{v}_extra_us_median"] = round((row[f"step_{v}_ms_median"] - row["step_off_ms_median"]) * 1e3, 1)
    return row


def kernel_table(path):
    """The advect kernels of a rocprofv3 --kernel-trace --stats CSV."""
    rows = []
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if "advect" not in name or "tracers" in name:
            continue
        avg = float(r.get("AverageNs") or r.get("AverageDurationNs")) / 1e3
        mn = float(r.get("MinNs") or r.get("MinDurationNs") or avg * 1e3) / 1e3
        rows.append({"kernel": name.split("(")[0].replace("void sfk::", ""), "calls": int(r.get("Calls", 0)),
                     "avg_us": round(avg, 1), "min_us": round(mn, 1)})
    return sorted(rows, key=lambda r: r["kernel"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["256:f32", "512:f32", "256:f64"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forms", action="store_true", help="one-field operators under SF_ADVECT_ROW = 0, 2, 3")
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of a run: print its advect kernels")
    a = ap.parse_args()
    if a.stats:
        for r in kernel_table(a.stats):
            print(json.dumps(r), flush=True)
        return
    for N, dtype in parse_cases(a.cases):
        head = {"grid": N, "dtype": dtype, "K": K, "reps": a.reps}
        if a.forms:
            for form in (0, 2, 3):
                os.environ["SF_ADVECT_ROW"] = str(form)
                fs = context(N, dtype)
                print(json.dumps(dict(head, SF_ADVECT_ROW=form, **time_operators(fs, a.reps, a.warmup, three=False))),
                      flush=True)
                fs.close()
            os.environ.pop("SF_ADVECT_ROW")
            continue
        fs = context(N, dtype)
        row = dict(head, **time_operators(fs, a.reps, a.warmup))
        row.update(time_steps(fs, a.reps, a.warmup))
        fs.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
