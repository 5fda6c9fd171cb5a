#!/usr/bin/env python3
"""Time sf_tracers_advect on one slab and on four (measurement aid, not the benchmark; docs/SPEC.md §6.1).

256^3 fp32 with a smooth random velocity that moves a tracer by up to ~1.5 planes per call (so that tracers cross
slab boundaries every call), n tracers spread over the box, three setups: one slab, four logical slabs with the
device-local transport, four logical slabs with RCCL send / receive to self (SF_FLAG_RCCL_SELF). Per call two
numbers, min and median over --reps calls after --warmup:
  dev_ms   device timer pair on slab 0's compute stream around the call (its chain ends with the arrivals kernel,
           which waits for its neighbour's move kernel and messages; the other slabs' arrivals may end a little later)
  wall_ms  host clock around the call + sf_sync (launch cost and the synchronisation included)

  python tools/tracer_bench.py                    # n = 1e5 and 1e6, all three setups
  python tools/tracer_bench.py --n 1000000 --setups p4-rccl-self --reps 5
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidsolvergpu_amd import solver as S  # noqa: E402

SETUPS = {"p1": (1, 0), "p4-copy": (4, 0), "p4-rccl-self": (4, S.SF_FLAG_RCCL_SELF)}


def smooth_field(N, rng, amp):
    """amp * a sum of a few low sine modes on the (N+2)^3 grid, fp32."""
    k = np.arange(N + 2, dtype=np.float64)
    f = np.zeros((N + 2,) * 3)
    for _ in range(3):
        a, b, c = rng.randint(1, 4, size=3)
        p = rng.uniform(0, 2 * np.pi, size=3)
        f += (np.sin(2 * np.pi * a * k / N + p[0])[None, None, :] * np.sin(2 * np.pi * b * k / N + p[1])[None, :, None]
              * np.sin(2 * np.pi * c * k / N + p[2])[:, None, None])
    return (amp * f / 3.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--setups", nargs="+", default=list(SETUPS))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=0, help="sf_tracers_set_capacity (0: default, the tracer count)")
    a = ap.parse_args()
    N, dt = a.grid, 0.1
    rng = np.random.RandomState(1)
    vmax = 1.5 / (dt * N)  # up to 1.5 planes per call
    fields = {"u": smooth_field(N, rng, vmax), "v": smooth_field(N, rng, vmax), "w": smooth_field(N, rng, vmax),
              "dens": smooth_field(N, rng, 1.0)}
    for setup in a.setups:
        P, flags = SETUPS[setup]
        fs = S.FluidSolver(N, dtype="f32", iters=4, dt=dt, nslabs_local=P, flags=flags)
        for k, f in fields.items():
            fs.upload(k, f)
        for n in a.n:
            pos = rng.uniform(0.5, N + 0.5, size=(n, 3)).astype(np.float32)
            fs.tracers_set(pos)
            if a.capacity > 0:
                fs.tracers_set_capacity(a.capacity)
            dev, wall = [], []
            for r in range(a.warmup + a.reps):
                fs.sync()
                fs.timer_start()
                t0 = time.perf_counter()
                fs.tracers_advect()
                ms = fs.timer_stop()
                fs.sync()
                t1 = time.perf_counter()
                if r >= a.warmup:
                    dev.append(ms)
                    wall.append((t1 - t0) * 1e3)
            info = fs.transport_info()
            print(json.dumps({"grid": N, "setup": setup, "n": n, "capacity": a.capacity or n, "reps": a.reps,
                              "dev_ms_min": round(min(dev), 4), "dev_ms_median": round(float(np.median(dev)), 4),
                              "wall_ms_min": round(min(wall), 4), "wall_ms_median": round(float(np.median(wall)), 4),
                              "transport": info["transport"], "owned": fs.tracers_owned()}), flush=True)
        fs.close()


if __name__ == "__main__":
    main()
