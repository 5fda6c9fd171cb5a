#!/usr/bin/env python3
"""Time volume rendering and light marching of docs/SPEC.md §12 (measurement aid, not the benchmark).

SPEC §5 inputs with bound sources (the benchmark's workload), K = 20, after two steps. sf_render and sf_light are
asynchronous, so they are timed on the device: the context's event pair around --reps calls, per call. Per case, in one
process:
  render_<axis>_ms / render_emit_<axis>_ms   one sf_render of the density along i, j, k, without / with an emission field
  light_<axis>_ms       one sf_light (the march and the set_bnd of its result)
  reduce_sum_ms         one sf_reduce(SF_RED_SUM) of the density, host wall time of the synchronising call, and
  reduce_rows_ms        its device time: the row pass, which reads the bytes a march reads with N^2 waves instead of
                        N^2 / 64, the fold of its records and their copy to the host
  *_over_reduce         march time / reduce_rows_ms
  snapshot_ms           sf_snapshot + sf_snapshot_read of the density: the path an image replaces (host wall time)
  render_read_ms        sf_render + sf_render_read (host wall time)
  step_ms               vel_step + dens_step per step, host wall time of --steps steps after a sync
  render1 / render10    the same loop with light + render + read after every step / every 10th step, and its share

--view times sf_render_view of docs/SPEC.md §13 instead: a 512 x 512 sf_view_frame image per case, for the directions
(0,0,1) (up (0,1,0)), (1,2,3) and (1,1,0), steps 1 and 0.5, without and with an emission field: ms per call and ns per
visited sample (counted exactly in numpy at N <= 256, else N^3 / (pix^2 step)). Yardsticks in the same process: sf_advect
of the density (the eight-gather kernel) and sf_render along k, both in ns per cell.

--camera times sf_render_camera of docs/SPEC.md §14 instead: a 512 x 512 sf_camera_frame image per case for three
cameras that look along (1,2,3) — far (20 N from the centre, the field of view that just holds the bounding sphere:
nearly parallel rays), near (1.5 N from the centre, 40 degrees) and inside (the eye in the box, 40 degrees) — steps 1 and
0.5, without and with an emission field, each next to sf_render_view along the same direction in the same process: ms per
call, ps per visited sample (counted in numpy in the arithmetic of §14 on every pixel at N <= 256 and on every fourth
pixel each way, times 16, above), and the ratio of the camera's ps per visited sample to the view's.

  python tools/render_bench.py                          # 64^3, 128^3, 256^3, 512^3 fp32 and 256^3 fp64
  python tools/render_bench.py --view                   # 256^3, 512^3 fp32 and 256^3 fp64
  python tools/render_bench.py --camera                 # 256^3, 512^3 fp32 and 256^3 fp64
  python tools/render_bench.py --cases 256:f32 --reps 5 # one case (e.g. under rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, DIFF, VISC, K, SIGMA = 0.1, 1e-4, 1e-4, 20, 4.0
AXES = "ijk"


def device_ms(fs, call, reps, warmup=2, trials=3):
    for _ in range(warmup):
        call()
    fs.sync()
    best = float("inf")
    for _ in range(trials):
        fs.timer_start()
        for _ in range(reps):
            call()
        best = min(best, fs.timer_stop() / reps)
    return best


def wall_ms(fs, call, reps, warmup=2):
    t = []
    for _ in range(warmup + reps):
        fs.sync()
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t[warmup:])


def loop_ms(fs, steps, every):
    fs.sync()
    t0 = time.perf_counter()
    for s in range(steps):
        fs.vel_step()
        fs.dens_step()
        if every and s % every == 0:
            fs.light("dens0", "dens", 2, 1, SIGMA)  # (dens0 is scratch between steps while its source is bound)
            fs.render("dens", "dens0", 1, 0, SIGMA)
    fs.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def make(N, dtype):
    from bench import upload_inputs
    from fluidsolvergpu_amd import solver as S

    fs = S.FluidSolver(N, dtype=dtype, iters=K, dt=DT, diff=DIFF, visc=VISC)
    upload_inputs(fs, N, DT)
    fs.bind_sources()
    for _ in range(2):
        fs.vel_step()
        fs.dens_step()
    fs.sync()
    return S, fs


def marches(S, fs, reps, axes, suffix=""):
    out = {}
    for axis in axes:
        for emit, tag in ((-1, "render"), (S.FIELD_IDS["dens0"], "render_emit")):
            p = S.SfRenderParams(axis=axis, from_high=0, sigma=SIGMA, dens=S.FIELD_IDS["dens"], emit=emit)
            out[f"{tag}_{AXES[axis]}{suffix}_ms"] = device_ms(fs, lambda: S.lib.sf_render(fs._h, C.byref(p)), reps)
        out[f"light_{AXES[axis]}{suffix}_ms"] = device_ms(fs, lambda: fs.light("dens0", "dens", axis, 0, SIGMA), reps)
    return out


def time_case(N, dtype, reps, steps):
    S, fs = make(N, dtype)
    out = {"grid": N, "dtype": dtype, "K": K, "reps": reps, "steps": steps}
    out.update(marches(S, fs, reps, (0, 1, 2)))
    red = C.c_double()
    out["reduce_sum_ms"] = wall_ms(fs, lambda: fs.reduce("sum", "dens"), reps)
    # (the call synchronises: one call per event pair, so that no host gap is timed)
    out["reduce_rows_ms"] = device_ms(fs, lambda: S.lib.sf_reduce(fs._h, S.SF_RED_SUM, S.FIELD_IDS["dens"], C.byref(red)),
                                      1, trials=reps)
    frame = np.zeros(fs.shape, fs.np_dtype)

    def snapshot():
        fs.snapshot(["dens"])
        fs.snapshot_read(0, frame)

    out["snapshot_ms"] = wall_ms(fs, snapshot, max(2, reps // 4))
    out["render_read_ms"] = wall_ms(fs, lambda: fs.render("dens", None, 1, 0, SIGMA), reps)
    loops = {0: [], 1: [], 10: []}
    for _ in range(3):  # best of three passes per variant, the variants interleaved
        for every in loops:
            loops[every].append(loop_ms(fs, steps, every))
    step, r1, r10 = (min(loops[e]) for e in (0, 1, 10))
    out.update(step_ms=step, render1_step_ms=r1, render10_step_ms=r10, render1_share=(r1 - step) / step,
               render10_share=(r10 - step) / step)
    fs.close()
    for k in [k for k in out if k.startswith(("render_", "light_")) and k.endswith("_ms") and k != "render_read_ms"]:
        out[k[:-3] + "_over_reduce"] = out[k] / out["reduce_rows_ms"]
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


VIEW_DIRS = [((0, 0, 1), (0, 1, 0)), ((1, 2, 3), (0, 0, 1)), ((1, 1, 0), (0, 0, 1))]


def visited_samples(N, T, f):
    """The number of visited samples of frame f (an SfViewParams) in the arithmetic of §13."""
    a = np.arange(f.width).astype(T)[None, :]
    b = np.arange(f.height).astype(T)[:, None]
    base = [((T(f.origin[c]) + a * T(f.du[c])) + b * T(f.dv[c])).astype(T) for c in range(3)]
    lo, hi, total = T(0.5), T(N) + T(0.5), 0
    for n in range(f.samples):
        vis = np.ones(base[0].shape, bool)
        for c in range(3):
            x = base[c] + T(n) * T(f.step[c])
            vis &= (x >= lo) & (x <= hi)
        total += int(np.count_nonzero(vis))
    return total


def time_view_case(N, dtype, reps, size=512):
    S, fs = make(N, dtype)
    T = fs.np_dtype
    out = {"grid": N, "dtype": dtype, "image": size, "reps": reps}
    cells = float(N) ** 3
    adv = device_ms(fs, lambda: fs.advect(0, "dens0", "dens", "u", "v", "w"), reps)
    rp = S.SfRenderParams(axis=2, from_high=0, sigma=SIGMA, dens=S.FIELD_IDS["dens"], emit=-1)
    rk = device_ms(fs, lambda: S.lib.sf_render(fs._h, C.byref(rp)), reps)
    out.update(advect_ms=adv, advect_ns_per_cell=adv * 1e6 / cells, render_k_ms=rk, render_k_ns_per_cell=rk * 1e6 / cells)
    for d, up in VIEW_DIRS:
        for step in (1.0, 0.5):
            f = fs.view_frame(d, up, size, size, step, SIGMA)
            pix = 3.0 ** 0.5 * N / size
            n = visited_samples(N, T, f) if N <= 256 else cells / (pix * pix * step)
            for emit, tag in ((-1, "view"), (S.FIELD_IDS["dens0"], "view_emit")):
                f.dens, f.emit = S.FIELD_IDS["dens"], emit
                ms = device_ms(fs, lambda: S.lib.sf_render_view(fs._h, C.byref(f)), reps)
                key = f"{tag}_{''.join(map(str, d))}_s{step}"
                out[key + "_ms"] = ms
                out[key + "_ns_per_sample"] = ms * 1e6 / n
                if emit < 0:
                    out[key + "_over_advect"] = (ms * 1e6 / n) / (adv * 1e6 / cells)
            out[f"samples_{''.join(map(str, d))}_s{step}"] = int(n)
    fs.close()
    return {k: (round(v, 5) if isinstance(v, float) else v) for k, v in out.items()}


CAMERA_DIR = (1.0, 2.0, 3.0)


def camera_visited(N, T, v, step_du, step_dv, stride=1):
    """The number of visited samples of a frame (v: its SfViewParams) in the arithmetic of §14, on every stride-th pixel
    each way, times stride^2."""
    a = np.arange(0, v.width, stride).astype(T)[None, :]
    b = np.arange(0, v.height, stride).astype(T)[:, None]
    base = [((T(v.origin[c]) + a * T(v.du[c])) + b * T(v.dv[c])).astype(T) for c in range(3)]
    r = [((T(v.step[c]) + a * T(step_du[c])) + b * T(step_dv[c])).astype(T) for c in range(3)]
    lo, hi, total = T(0.5), T(N) + T(0.5), 0
    for n in range(v.samples):
        vis = np.ones(base[0].shape, bool)
        for c in range(3):
            x = base[c] + T(n) * r[c]
            vis &= (x >= lo) & (x <= hi)
        total += int(np.count_nonzero(vis))
    return total * stride * stride


def time_camera_case(N, dtype, reps, size=512):
    S, fs = make(N, dtype)
    T = fs.np_dtype
    out = {"grid": N, "dtype": dtype, "image": size, "reps": reps}
    stride = 1 if N <= 256 else 4
    d = np.array(CAMERA_DIR) / np.linalg.norm(CAMERA_DIR)
    c = (N + 1) / 2.0
    half = float(np.degrees(np.arctan((3.0 ** 0.5 * N / 2.0) / (20.0 * N))))
    cameras = {"far": (c - 20.0 * N * d, 2.0 * half), "near": (c - 1.5 * N * d, 40.0), "inside": (c - 0.2 * N * d, 40.0)}
    zero = (0.0, 0.0, 0.0)
    for step in (1.0, 0.5):
        v = fs.view_frame(CAMERA_DIR, (0, 0, 1), size, size, step, SIGMA)
        nv = camera_visited(N, T, v, zero, zero, stride)
        ortho = {}
        for emit, tag in ((-1, "plain"), (S.FIELD_IDS["dens0"], "emit")):
            v.dens, v.emit = S.FIELD_IDS["dens"], emit
            ortho[tag] = device_ms(fs, lambda: S.lib.sf_render_view(fs._h, C.byref(v)), reps)
            out[f"view_{tag}_s{step}_ms"] = ortho[tag]
            out[f"view_{tag}_s{step}_ps_per_sample"] = ortho[tag] * 1e9 / nv
        out[f"view_samples_s{step}"] = nv
        for name, (eye, fov) in cameras.items():
            f = fs.camera_frame(eye, (c, c, c), (0, 0, 1), fov, size, size, step, SIGMA)
            n = camera_visited(N, T, f.view, f.step_du, f.step_dv, stride)
            out[f"{name}_samples_s{step}"] = n
            out[f"{name}_passes_s{step}"] = fs.camera_passes(f)
            for emit, tag in ((-1, "plain"), (S.FIELD_IDS["dens0"], "emit")):
                f.view.dens, f.view.emit = S.FIELD_IDS["dens"], emit
                ms = device_ms(fs, lambda: S.lib.sf_render_camera(fs._h, C.byref(f)), reps)
                key = f"{name}_{tag}_s{step}"
                out[key + "_ms"] = ms
                out[key + "_ps_per_sample"] = ms * 1e9 / n
                out[key + "_over_view"] = (ms / n) / (ortho[tag] / nv)
    fs.close()
    return {k: (round(v, 5) if isinstance(v, float) else v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--view", action="store_true", help="time sf_render_view (SPEC §13) instead")
    ap.add_argument("--camera", action="store_true", help="time sf_render_camera (SPEC §14) next to sf_render_view instead")
    ap.add_argument("--cases", nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if a.cases is None:
        a.cases = ["256:f32", "512:f32", "256:f64"] if (a.view or a.camera) else ["64:f32", "128:f32", "256:f32", "512:f32", "256:f64"]
    for c in a.cases:
        n, t = c.split(":")
        if a.camera:
            out = time_camera_case(int(n), t, a.reps)
        else:
            out = time_view_case(int(n), t, a.reps) if a.view else time_case(int(n), t, a.reps, a.steps)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
