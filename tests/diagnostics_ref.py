"""numpy reference of docs/SPEC.md §10 "Reductions and diagnostics", written from the SPEC text. It does not call the
library. Fields are (N+2, N+2, N+2) arrays indexed [k, j, i] of float32 or float64; every result is a Python float
(a double) whose bits the library must reproduce.

The sum tree: 64 lane accumulators per row (lane l takes cells i = 1 + W*(l + 64 m) + e in increasing i), folded by
halving; the N row partials of a plane padded with +0.0 to a power of two and folded by halving; the plane partials
added in increasing k. Vectorised over rows and planes: the lane loop runs ceil(N / (64 W)) * W additions.
"""
import math

import numpy as np

OPS = ("sum", "sum_sq", "min", "max", "max_abs", "count_nonfinite")
SUM_KIND, MIN_KIND, MAX_KIND = 0, 1, 2
KIND = {"sum": SUM_KIND, "sum_sq": SUM_KIND, "count_nonfinite": SUM_KIND, "min": MIN_KIND, "max": MAX_KIND,
        "max_abs": MAX_KIND}
LANES = 64


def vec_width(dtype):
    """W = 16 / sizeof(T)."""
    return 16 // np.dtype(dtype).itemsize


def pad_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def halve(c):
    """Fold the last axis (a power of two long) by halving: c[l] += c[l + s] for s = len/2 ... 1."""
    c = c.copy()
    s = c.shape[-1] // 2
    while s >= 1:
        c[..., :s] = c[..., :s] + c[..., s:2 * s]
        s //= 2
    return c[..., 0]


def row_partials(terms, W):
    """terms: (nk, N, N) doubles [k, j, i-1] -> R(j, k) as (nk, N)."""
    nk, N, _ = terms.shape
    nm = -(-N // (LANES * W))
    t = np.zeros((nk, N, nm * LANES * W), np.float64)  # cells past N add +0.0
    t[:, :, :N] = terms
    t = t.reshape(nk, N, nm, LANES, W)
    c = np.zeros((nk, N, LANES), np.float64)
    for m in range(nm):
        for e in range(W):
            c = c + t[:, :, m, :, e]
    return halve(c)


def plane_partials(terms, W):
    """terms: (nk, N, N) -> Pl(k) as (nk,)."""
    R = row_partials(terms, W)
    nk, N = R.shape
    a = np.zeros((nk, pad_pow2(N)), np.float64)
    a[:, :N] = R
    return halve(a)


def total(planes):
    """Sequential sum in increasing k from +0.0."""
    t = 0.0
    with np.errstate(all="ignore"):
        for x in np.asarray(planes, np.float64):
            t = t + float(x)
    return float(t)


def _finite_min(x, axis):
    return np.where(np.isfinite(x), x, np.inf).min(axis=axis)


def _finite_max(x, axis, start):
    return np.where(np.isfinite(x), x, start).max(axis=axis, initial=start)


def plane_records(op, x):
    """Per-plane values of reduce(op, x) for the interior planes of x (every plane of x but its first and last), as
    doubles: what one slab produces for the planes it owns. x: (nk + 2, N + 2, N + 2)."""
    dtype = x.dtype
    inner = x[1:-1, 1:-1, 1:-1]
    with np.errstate(all="ignore"):
        if op == "sum":
            return plane_partials(inner.astype(np.float64), vec_width(dtype))
        if op == "sum_sq":
            d = inner.astype(np.float64)
            return plane_partials(d * d, vec_width(dtype))
        if op == "count_nonfinite":
            return (~np.isfinite(inner)).sum(axis=(1, 2)).astype(np.float64)
        if op == "min":
            return _finite_min(inner, (1, 2)).astype(np.float64)
        if op == "max":
            return _finite_max(inner, (1, 2), -np.inf).astype(np.float64)
        if op == "max_abs":
            return _finite_max(np.abs(inner), (1, 2), 0.0).astype(np.float64)
    raise ValueError(op)


def fold(kind, records):
    """The fold over global k of per-plane values: sequential sum, or select; a zero minimum / maximum is +0."""
    r = np.asarray(records, np.float64)
    if kind == SUM_KIND:
        return total(r)
    m = float(r.min()) if kind == MIN_KIND else float(r.max())
    return m + 0.0


def reduce(op, x):
    """reduce(op, x) over the interior cells of the (N+2)^3 field x."""
    return fold(KIND[op], plane_records(op, x))


def reduce_slabs(op, x, P):
    """The same through P slabs: each computes the records of its own planes from its planes and one ghost plane either
    side; the records are concatenated in global k order and folded. Same bits as reduce() for every P dividing N."""
    N = x.shape[0] - 2
    assert N % P == 0
    nzl = N // P
    recs = [plane_records(op, x[s * nzl:(s + 1) * nzl + 2]) for s in range(P)]
    return fold(KIND[op], np.concatenate(recs))


DIAG_KINDS = (("mass", SUM_KIND), ("kin", SUM_KIND), ("nonfinite", SUM_KIND), ("dens_min", MIN_KIND),
              ("dens_max", MAX_KIND), ("speed2", MAX_KIND), ("max_div", MAX_KIND), ("cfl_x", MAX_KIND),
              ("cfl_y", MAX_KIND), ("cfl_z", MAX_KIND))


def diag_plane_records(u, v, w, dens, dt, N):
    """Per-plane records of the state diagnostics for the interior planes of the given (nk + 2, N + 2, N + 2) arrays
    (one ghost / shell plane either side, as stored). dict name -> (nk,) doubles."""
    T = u.dtype.type
    W = vec_width(u.dtype)
    c_div = T(-0.5) * (T(1) / T(N))
    dt0 = T(dt) * T(N)
    c = (slice(1, -1),) * 3
    with np.errstate(all="ignore"):
        du = u[1:-1, 1:-1, 2:] - u[1:-1, 1:-1, :-2]
        dv = v[1:-1, 2:, 1:-1] - v[1:-1, :-2, 1:-1]
        dw = w[2:, 1:-1, 1:-1] - w[:-2, 1:-1, 1:-1]
        div = np.abs(c_div * ((du + dv) + dw))
        assert div.dtype == u.dtype
        ud, vd, wd = (f[c].astype(np.float64) for f in (u, v, w))
        s2 = (ud * ud + vd * vd) + wd * wd
        bad = ~(np.isfinite(u[c]) & np.isfinite(v[c]) & np.isfinite(w[c]) & np.isfinite(dens[c]))
        return {
            "mass": plane_partials(dens[c].astype(np.float64), W),
            "kin": plane_partials(s2, W),
            "nonfinite": bad.sum(axis=(1, 2)).astype(np.float64),
            "dens_min": _finite_min(dens[c], (1, 2)).astype(np.float64),
            "dens_max": _finite_max(dens[c], (1, 2), -np.inf).astype(np.float64),
            "speed2": _finite_max(s2, (1, 2), 0.0),
            "max_div": _finite_max(div, (1, 2), 0.0).astype(np.float64),
            "cfl_x": _finite_max(np.abs(dt0 * u[c]), (1, 2), 0.0).astype(np.float64),
            "cfl_y": _finite_max(np.abs(dt0 * v[c]), (1, 2), 0.0).astype(np.float64),
            "cfl_z": _finite_max(np.abs(dt0 * w[c]), (1, 2), 0.0).astype(np.float64),
        }


def diag_fold(records, N):
    r = {name: fold(kind, records[name]) for name, kind in DIAG_KINDS}
    return {
        "mass": r["mass"], "dens_min": r["dens_min"], "dens_max": r["dens_max"],
        "kinetic": (0.5 * r["kin"]) / float(N ** 3),
        "max_speed": math.sqrt(r["speed2"]), "max_div": r["max_div"],
        "cfl_x": r["cfl_x"], "cfl_y": r["cfl_y"], "cfl_z": r["cfl_z"],
        "cfl": max(r["cfl_x"], r["cfl_y"], r["cfl_z"]), "nonfinite": int(r["nonfinite"]),
    }


def diagnostics(u, v, w, dens, dt, P=1):
    """State diagnostics of SPEC §10 of full (N+2)^3 fields, through P slabs (same bits for every P dividing N)."""
    N = u.shape[0] - 2
    assert N % P == 0
    nzl = N // P
    parts = [diag_plane_records(*(f[s * nzl:(s + 1) * nzl + 2] for f in (u, v, w, dens)), dt, N) for s in range(P)]
    return diag_fold({name: np.concatenate([p[name] for p in parts]) for name, _ in DIAG_KINDS}, N)


def sum_path_additions(N, dtype):
    """Additions on the longest path from a cell to the total: the lane's sequential adds, the 6 halving steps of the
    wave, log2(pad(N)) halving steps of the plane, N sequential adds over k."""
    W = vec_width(dtype)
    return -(-N // (LANES * W)) * W + 6 + int(math.log2(pad_pow2(N))) + N


def bits(x):
    """The 64 bits of a double (for exact comparison; every NaN compares equal to every NaN: its payload is
    unspecified)."""
    x = float(x)
    if math.isnan(x):
        return "nan"
    return np.float64(x).view(np.uint64).item()
