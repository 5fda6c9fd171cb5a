#!/usr/bin/env python3
"""Time the full step (vel_step + dens_step) with the forces of docs/SPEC.md §8 off, vorticity confinement only, and
vorticity confinement plus buoyancy (measurement aid, not the benchmark).

SPEC §5 inputs with bound sources (the benchmark's workload), K = 20. The variants alternate step by step in one
process; per variant the device-timer min and median over --reps steps after --warmup, and the overhead of the forces
(variant minus off). The copy ceiling of the same run (sf_measure_copy_bandwidth, 1 GiB) turns compulsory bytes into
a time. What vel_step adds with a force on, in words per interior cell:
  vorticity_mag_kernel  4   (u, v, w read, |omega| written)
  add_forces_kernel     10  (u, v, w, |omega|, the three bound sources read, the three x0 slots written), +1 dens
  add_source unfused    6   (the bound-source step folds add_source into diffuse's first pass, 4 words per field; the
                             forces path runs add_source and a plain first pass instead, 6)

  python tools/forces_bench.py                                 # 256^3 fp32, 512^3 fp32, 256^3 fp64
  python tools/forces_bench.py --cases 256:f32 --reps 5        # one case (e.g. under rocprofv3 --kernel-trace --stats)
  python tools/forces_bench.py --stats kernel_stats.csv --cases 256:f32 --gbps 6100   # per-kernel table of that run
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
VARIANTS = {"off": dict(eps=0.0, beta=0.0), "vort": dict(eps=0.25, beta=0.0), "vort+buoy": dict(eps=0.25, beta=0.8)}
WORDS = {"vorticity_mag_kernel": 4, "add_forces_kernel<vort>": 10, "add_forces_kernel<vort+buoy>": 11}
STAGE_WORDS = {"vort": 4 + 10 + 6, "vort+buoy": 4 + 11 + 6}


def parse_cases(cases):
    out = []
    for c in cases:
        n, t = c.split(":")
        out.append((int(n), t))
    return out


def compulsory_us(N, dtype, words, gbps):
    return words * float(N) ** 3 * (4 if dtype == "f32" else 8) / (gbps * 1e9) * 1e6


def time_case(N, dtype, reps, warmup):
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
    del a
    fs.bind_sources()
    times = {v: [] for v in VARIANTS}
    for r in range(warmup + reps):
        for v, c in VARIANTS.items():
            fs.set_vorticity_confinement(c["eps"])
            fs.set_buoyancy(c["beta"], 0.5, 1)
            fs.sync()
            fs.timer_start()
            fs.vel_step()
            fs.dens_step()
            ms = fs.timer_stop()
            if r >= warmup:
                times[v].append(ms)
    fs.sync()
    gbps = fs.copy_bandwidth_gbps(1 << 30, 5)
    fs.close()
    row = {"grid": N, "dtype": dtype, "K": K, "reps": reps, "copy_gbps": round(gbps, 1)}
    off_min, off_med = min(times["off"]), float(np.median(times["off"]))
    for v, t in times.items():
        row[f"{v}_ms_min"] = round(min(t), 4)
        row[f"{v}_ms_median"] = round(float(np.median(t)), 4)
        if v != "off":
            over_min = (min(t) - off_min) * 1e3
            over_med = (float(np.median(t)) - off_med) * 1e3
            bound = compulsory_us(N, dtype, STAGE_WORDS[v], gbps)
            row[f"{v}_overhead_us_min"] = round(over_min, 1)
            row[f"{v}_overhead_us_median"] = round(over_med, 1)
            row[f"{v}_compulsory_us"] = round(bound, 1)
            row[f"{v}_overhead_over_compulsory"] = round(over_med / bound, 2)
    return row


def kernel_table(path, N, dtype, gbps):
    """Per-kernel averages of a rocprofv3 --kernel-trace --stats CSV of ONE case against their compulsory bytes."""
    T = "float" if dtype == "f32" else "double"
    rows = []
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if T not in name:
            continue
        if "vorticity_mag_kernel" in name:
            key = "vorticity_mag_kernel"
        elif "add_forces_kernel" in name:
            key = "add_forces_kernel<vort+buoy>" if f"<{T}, true, true" in name else (
                "add_forces_kernel<vort>" if f"<{T}, true, false" in name else None)
        else:
            continue
        if key is None:
            continue
        avg = float(r.get("AverageNs") or r.get("AverageDurationNs")) / 1e3
        mn = float(r.get("MinNs") or r.get("MinDurationNs") or avg * 1e3) / 1e3
        bound = compulsory_us(N, dtype, WORDS[key], gbps)
        rows.append({"kernel": name, "calls": int(r.get("Calls", 0)), "avg_us": round(avg, 1), "min_us": round(mn, 1),
                     "compulsory_us": round(bound, 1), "avg_over_compulsory": round(avg / bound, 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["256:f32", "512:f32", "256:f64"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of a run of ONE case: print the per-kernel table")
    ap.add_argument("--gbps", type=float, default=0.0, help="copy ceiling of that run (GB/s of traffic)")
    a = ap.parse_args()
    cases = parse_cases(a.cases)
    if a.stats:
        N, dtype = cases[0]
        for r in kernel_table(a.stats, N, dtype, a.gbps):
            print(json.dumps(dict(grid=N, dtype=dtype, copy_gbps=a.gbps, **r)), flush=True)
        return
    for N, dtype in cases:
        print(json.dumps(time_case(N, dtype, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
