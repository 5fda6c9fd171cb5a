"""The batched protocol of docs/SPEC.md §11 "Where the scalars are computed" as a numpy model, and the inputs that stop a
solve, shared by tests/test_pressure_cg_device_ref.py (CPU: results do not depend on check_every, the inputs tell three
wrong protocols from the right one) and tests/test_pressure_cg_device_gpu.py (GPU: the library against the reference).

The model is layered on tests/pressure_cg_ref.py, which it imports unchanged: every field expression and every sum is
the reference's. What it adds is the schedule: a state (rho0, rho, last, aT, bT, status, iterations, active) that only
the four stages write, row kernels that do nothing once active == 0, iterations enqueued in batches of
min(m, max_iters - n) and one read-back of the state per batch. It does not call the library."""
import math

import numpy as np

import pressure_cg_ref as R
import shape_cases as C

I = R.I
MUTANTS = ("no_freeze", "count_enqueued", "late_freeze")


def project_cg_batched(u, v, w, tol, max_iters, m, mut=None):
    """R.project_cg through the batched protocol with check_every = m >= 1. Returns its dict plus host_waits.
    Mutants (None: the protocol of the SPEC):
      no_freeze       CONVERGED sets the status but leaves the solve active: the iterations enqueued after it run
      count_enqueued  `iterations` counts every enqueued iteration, stopped or not
      late_freeze     a delta breakdown stops the solve after cg_update instead of before it"""
    assert m >= 1
    dtype = u.dtype
    T = dtype.type
    N = u.shape[0] - 2
    u, v, w = u.copy(), v.copy(), w.copy()
    st = {"status": R.MAX_ITERS, "iterations": 0, "active": 0}
    with np.errstate(all="ignore"):
        p, div = R.divergence(u, v, w)
        st["mu"] = T(R.tree_sum(div[I, I, I].astype(np.float64), dtype) / float(N) ** 3)  # STAGE_MU
        r = div[I, I, I] - st["mu"]  # cg_init: not gated
        d = np.zeros_like(u)
        d[I, I, I] = r
        R.set_bnd(0, d)
        s = R.dot(r, r, dtype)  # STAGE_RHO0
        st["rho0"] = st["rho"] = st["last"] = s
        st["status"] = R.CONVERGED if s == 0.0 else (R.MAX_ITERS if math.isfinite(s) else R.BREAKDOWN)
        st["active"] = 1 if (s != 0.0 and math.isfinite(s)) else 0
        st["aT"] = st["bT"] = T(0)
        q = np.zeros_like(r)
        rec = 0.0  # the row records' sum, as the last kernel that wrote them left it
        n = waits = 0
        while True:
            for _ in range(min(m, max_iters - n)):
                n += 1
                if st["active"]:  # cg_apply_dot
                    q = R.apply_A(d)
                    rec = R.dot(d[I, I, I], q, dtype)
                freeze_late = False
                if st["active"]:  # STAGE_DELTA
                    if not rec > 0.0:
                        st["status"] = R.BREAKDOWN
                        freeze_late = mut == "late_freeze"
                        st["active"] = 1 if freeze_late else 0
                    if st["active"]:
                        st["aT"] = T(np.float64(st["rho"]) / np.float64(rec))
                if st["active"]:  # cg_update
                    p[I, I, I] = p[I, I, I] + st["aT"] * d[I, I, I]
                    r = r - st["aT"] * q
                    rec = R.dot(r, r, dtype)
                if freeze_late:
                    st["active"] = 0
                if st["active"]:  # STAGE_RHO
                    st["last"] = rec
                    st["iterations"] += 1
                    if not math.isfinite(rec):
                        st["status"], st["active"] = R.BREAKDOWN, 0
                    elif rec <= (tol * tol) * st["rho0"]:
                        st["status"], st["active"] = R.CONVERGED, (1 if mut == "no_freeze" else 0)
                    else:
                        st["bT"] = T(rec / st["rho"])
                        st["rho"] = rec
                elif mut == "count_enqueued":
                    st["iterations"] += 1
                if st["active"]:  # cg_direction
                    d[I, I, I] = r + st["bT"] * d[I, I, I]
                    R.set_bnd(0, d)
            waits += 1  # the read-back
            if not st["active"] or n >= max_iters:
                break
        status = R.MAX_ITERS if st["active"] else st["status"]
        R.set_bnd(0, p)
        R.subtract_gradient(u, v, w, p)
        rho0, last = st["rho0"], st["last"]
        rel = 0.0 if rho0 == 0.0 else math.sqrt(last / rho0) if last / rho0 >= 0 else float("nan")
    return {"u": u, "v": v, "w": w, "p": p, "div": div, "status": status, "iterations": st["iterations"],
            "rel_residual": rel, "host_waits": waits}


# ---- inputs that stop a solve --------------------------------------------------------------------------------------
def zero_velocity(N, dtype):
    """test_pressure_cg_shapes_gpu.test_zero_velocity_with_a_negative_zero's: a fixed point of the three set_bnd with one
    interior -0. rho0 == 0: CONVERGED with 0 iterations."""
    u, v, w = (np.zeros((N + 2,) * 3, dtype) for _ in range(3))
    u[N // 2, min(3, N), N] = -0.0
    for b, f in ((1, u), (2, v), (3, w)):
        R.set_bnd(b, f)
    return u, v, w


def nan_velocity(N, dtype, seed):
    """A NaN in u: it reaches div, the mean and so every cell of r: rho0 is a NaN, BREAKDOWN with 0 iterations."""
    u, v, w = C.cg_velocity(N, dtype, seed)
    u[N // 2, 1, N] = np.nan
    return u, v, w


def inf_velocity(N, dtype, seed, value):
    """test_pressure_cg_shapes_gpu.test_an_infinite_cell_is_a_status's input."""
    u, v, w = C.cg_velocity(N, dtype, seed)
    w[N // 2, min(3, N), min(5, N)] = value
    return u, v, w


# (N, dtype, seed of shape_cases.cg_velocity, iterations): solves that end in a delta breakdown. With tol = 1e-200 (tol * tol
# underflows to 0: only rho' == 0 would converge) a small grid is iterated far below its residual floor until d.Ad comes
# out <= 0 by rounding: BREAKDOWN after `iterations` completed iterations, rel_residual finite, and p as the last completed
# update left it — cg_update must not run with alpha = (T)(rho / delta) for that delta.
DELTA_TOL, DELTA_MAX = 1e-200, 40
DELTA_BREAKDOWN = [(2, np.float32, 2, 6), (4, np.float32, 2, 22), (2, np.float64, 3, 6), (3, np.float64, 3, 16)]


def tol_stopping_at(u, v, w, it):
    """A tol with which the reference reports CONVERGED at iteration `it` exactly: the geometric mean of the relative
    residuals after it - 1 and after it iterations (which must fall between them)."""
    rel = [R.project_cg(u, v, w, 1e-300, k)["rel_residual"] for k in (it - 1, it)]
    assert rel[1] < rel[0], rel
    tol = math.sqrt(rel[0] * rel[1])
    assert rel[1] < tol < rel[0]
    return tol


STOP_N, STOP_TOL = 12, 1e-3  # (12: the stop cases also run on 4 slabs)


def stop_inputs():
    """name -> (u, v, w, tol, max_iters): every way a solve can stop, in both precisions. Shared by the CPU and the GPU
    file, so that the case a mutant is caught on there is the case that runs here."""
    out = {}
    for dtype in C.DTYPES:
        t = C.dname(dtype)
        N = STOP_N
        out[f"zero-{t}"] = (*zero_velocity(N, dtype), STOP_TOL, 20)
        out[f"nan-{t}"] = (*nan_velocity(N, dtype, 40 + N), STOP_TOL, 20)
        out[f"+inf-{t}"] = (*inf_velocity(N, dtype, 40 + N, np.inf), STOP_TOL, 20)
        out[f"-inf-{t}"] = (*inf_velocity(N, dtype, 40 + N, -np.inf), STOP_TOL, 20)
        vel = C.cg_velocity(N, dtype, 60 + N)
        out[f"max_iters0-{t}"] = (*vel, STOP_TOL, 0)
        out[f"max_iters1-{t}"] = (*vel, STOP_TOL, 1)
        out[f"tol1e30-{t}"] = (*vel, 1e30, 50)
        out[f"tol1e-200-{t}"] = (*vel, 1e-200, 12)
        out[f"stop_at_2-{t}"] = (*vel, tol_stopping_at(*vel, 2), 8)
    for N, dtype, seed, _ in DELTA_BREAKDOWN:
        out[f"delta-N{N}-{C.dname(dtype)}"] = (*C.cg_velocity(N, dtype, seed), DELTA_TOL, DELTA_MAX)
    return out
