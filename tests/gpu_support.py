"""What the GPU suites (tests/test_*_gpu.py) share: the constants of the step, the case table of the single operators,
the context factory, the comparison, the input builders, the checks against the numpy references and the fixtures
that select a kernel form. A test module imports what it needs from here and from the reference modules, never from
another test module. Importing this module needs no GPU and no libsfgpu.so."""
import json
import socket

import numpy as np
import pytest

import diagnostics_ref as D
import forces_ref as F
import maccormack_ref as MC
import oracle_lib as O
import pressure_cg_ref as R
import pressure_pcg_ref as Q
import stable_ref as S3
from abi_header import ROOT  # noqa: F401  (the repository root; defined there once, re-exported)
from bench import analytic_planes  # (the benchmark inputs, docs/SPEC.md §5)
from shape_cases import DT, DTYPES, dname  # noqa: F401  (DT and DTYPES are defined there once; re-exported)

DIFF, VISC = 1e-4, 1e-4
NAMES = ("u", "v", "w", "u0", "v0", "w0", "dens", "dens0")
USER = {"u0": "user0", "v0": "user1", "w0": "user2", "dens0": "user3"}
STATE = ("u", "v", "w", "dens")
DTYPE_IDS = ["f32", "f64"]
# (N, P, transport) of the single-operator tests of SPEC §8 to §11
OPERATOR_CASES = [(17, 1, "copy"), (40, 1, "copy"), (40, 2, "copy"), (40, 4, "rccl-self"), (40, 5, "copy"),
                  (64, 1, "copy"), (64, 2, "rccl-self"), (64, 4, "copy")]
OPERATOR_IDS = [f"N{n}-P{p}-{t}" for n, p, t in OPERATOR_CASES]
# the switch settings a vel_step with CG selected is run under (test_pressure_cg_shapes_gpu; the preconditioned step of
# test_pressure_pcg_plans_gpu adds its own to them)
CG_STEP_SETTINGS = [{"SF_MARCH_MINCELLS_K": "0"},  # K = 9: the marching first pass leaves a dead i-shell in front of project_cg
                    {"SF_MARCH": "0"}, {"SF_ISHELL": "0"}, {"SF_ISHELL": "2"}, {"SF_GHOST": "1"}, {"SF_GHOST": "3"},
                    {"SF_FUSE2": "0"}, {"SF_FUSE_SRC": "0"}, {"SF_HALO_STREAM": "2"}, {"SF_SPLIT": "0"},
                    {"SF_SPLIT_FIELDS": "0"}, {"SF_ADVECT_ROW": "2"}, {"SF_GRAPH": "1"}]


def S():
    from fluidsolvergpu_amd import solver

    return solver


# ---- contexts ----------------------------------------------------------------------------------------------------
# Halo transport between the logical slabs of one context: the device-local copy kernel, or a real single-rank RCCL
# communicator with grouped ncclSend / ncclRecv to self (SF_FLAG_RCCL_SELF: the calls, streams and fences of the
# multi-process exchange, executed on the one GPU a test box has).
def make(N, dtype, K=4, P=1, transport="copy", **kw):
    """A context of P logical slabs. P = 1 passes no nslabs_local; flags only for rccl-self on P >= 2. The parity family
    passes **slab_kw(transport, P) instead, which goes through unchanged."""
    if P > 1:
        kw["nslabs_local"] = P
        if transport == "rccl-self":
            kw["flags"] = S().SF_FLAG_RCCL_SELF
    return S().FluidSolver(N, dtype=dname(dtype), iters=K, dt=DT, diff=DIFF, visc=VISC, **kw)


def slab_kw(transport, P):
    return {"nslabs_local": P, "flags": 2} if (transport == "rccl-self" and P >= 2) else {"nslabs_local": P}


def check_transport(fs, transport, P):
    """The context really used the transport the test asked for (and RCCL groups were issued)."""
    info = fs.transport_info()
    if P < 2:
        assert info["transport"] == "none"
    elif transport == "rccl-self":
        assert info["transport"] == "rccl-self" and info["rccl_groups"] > 0, info
    else:
        assert info["transport"] == "copy" and info["rccl_groups"] == 0, info


# ---- the comparison ----------------------------------------------------------------------------------------------
def _raise_on(differ, got, want, what):
    bad = np.argwhere(differ)
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at [k,j,i]={bad[0]}: got {got[at]!r} "
                             f"want {want[at]!r}")


def assert_same_bits(got, want, what, nan_ok=False):
    """Exact equality of the bits: the sign of a zero and the payload of a NaN included. nan_ok: NaN in the same entries,
    their payloads not compared; every other entry the same bits."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    uint = np.uint32 if got.dtype == np.float32 else np.uint64
    differ = got.view(uint) != want.view(uint)
    if nan_ok:
        differ &= ~(np.isnan(got) & np.isnan(want))
    _raise_on(differ, got, want, what)


# ---- inputs ------------------------------------------------------------------------------------------------------
def rand_fields(N, dtype, seed, scale=0.2):
    rng = np.random.RandomState(seed)
    return {n: (scale * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in NAMES}


def small_velocity(f, N, dtype):
    """|dt*N*w| < 1 so one ghost plane suffices (SPEC §4)."""
    lim = 0.9 / (DT * N)
    for n in ("u", "v", "w", "u0", "v0", "w0"):
        f[n] = np.clip(f[n], -lim / 4, lim / 4).astype(dtype)
    return f


def random_fields(N, dtype, seed, vel=0.05):
    """Random state whose traces stay within one plane (|dt*N*w| < 1) for the decomposed contexts."""
    rng = np.random.RandomState(seed)
    f = {n: (0.2 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in NAMES}
    for n in ("u", "v", "w"):
        f[n] = (vel * rng.standard_normal((N + 2,) * 3)).astype(dtype)
    return f


def bench_state(N, dtype):
    """The benchmark inputs (docs/SPEC.md §5): (state with its shells set, bound sources)."""
    a = analytic_planes(N, 0, N + 2, DT, dtype)
    f = {"u": a["u"], "v": a["v"], "w": a["w"], "dens": a["dens"]}
    for b, n in ((1, "u"), (2, "v"), (3, "w"), (0, "dens")):
        O.set_bnd(b, f[n])
    src = {"u0": a["su"], "v0": a["sv"], "w0": a["sw"], "dens0": a["sd"]}
    return f, src


class Cache:
    """References keyed by case, a few kept (the cases of one key run one after another)."""

    def __init__(self, keep=2):
        self.keep, self.items = keep, {}

    def get(self, key, build):
        if key not in self.items:
            while len(self.items) >= self.keep:
                self.items.pop(next(iter(self.items)))
            self.items[key] = build()
        return self.items[key]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- a context against the references ----------------------------------------------------------------------------
def upload_all(fs, f):
    for n, a in f.items():
        fs.upload(n, a)


def check_all(fs, want, what, names=NAMES):
    fs.sync()
    for n in names:
        assert_same_bits(fs.download(n), want[n], f"{what}: {n}")


def set_forces(fs, eps=0.0, beta=0.0, ambient=0.0, axis=1):
    fs.set_vorticity_confinement(eps)
    fs.set_buoyancy(beta, ambient, axis)


def check_reduce(fs, slot, x, what):
    for op in D.OPS:
        got, want = fs.reduce(op, slot), D.reduce(op, x)
        print(f"{what} {op}: got {got!r} want {want!r}")
        assert D.bits(got) == D.bits(want), f"{what}: {op}: got {got!r} want {want!r}"


def check_diag(fs, f, what):
    got, want = fs.diagnostics(), D.diagnostics(f["u"], f["v"], f["w"], f["dens"], DT)
    print(f"{what}: {got}")
    assert set(got) == set(want)
    for name in want:
        assert D.bits(got[name]) == D.bits(want[name]), f"{what}: {name}: got {got[name]!r} want {want[name]!r}"
    assert isinstance(got["nonfinite"], int)
    return got


def check_solve(fs, u, v, w, tol, max_iters, what, want=None):
    """Uploads u, v, w, runs sf_project_cg into (u0, v0) and compares everything with the reference (`want`, if the
    caller has computed R.project_cg of these arguments already). Returns it."""
    for n, a in (("u", u), ("v", v), ("w", w)):
        fs.upload(n, a)
    info = fs.project_cg("u", "v", "w", "u0", "v0", tol, max_iters)
    fs.sync()
    if want is None:
        want = R.project_cg(u, v, w, tol, max_iters)
    print(f"{what}: got {info} want status {want['status']} iterations {want['iterations']} rel {want['rel_residual']!r}")
    assert info["solver"] == S().SF_PRESSURE_CG
    assert (info["status"], info["iterations"]) == (want["status"], want["iterations"]), what
    assert D.bits(info["rel_residual"]) == D.bits(want["rel_residual"]), what
    for slot, name in (("u", "u"), ("v", "v"), ("w", "w"), ("u0", "p"), ("v0", "div")):
        assert_same_bits(fs.download(slot), want[name], f"{what}: {name}")
    got = fs.poisson_residual("u0", "v0")
    assert D.bits(got) == D.bits(R.poisson_residual(want["p"], want["div"])), what
    return want


def reference_vel_step(f, K, tol, max_iters, m, sources=None, forces=None, maccormack=False):
    """SPEC §3 vel_step on copies of the velocity fields of f, both projections Q.project_cg with m sweeps (SPEC §11
    "vel_step with the solver selected"). sources: bound sources {"u0": array, ...}, which replace the x0 fields first
    (sf_bind_sources); forces: the keywords of forces_ref.add_forces (SPEC §8; reads f["dens"]); maccormack: the
    advection of SPEC §9. Returns the second projection's outcome, whose u, v, w are the step's."""
    u, v, w, u0, v0, w0 = (f[n].copy() for n in ("u", "v", "w", "u0", "v0", "w0"))
    if sources:
        u0, v0, w0 = (sources[n].copy() for n in ("u0", "v0", "w0"))
    if forces:
        F.add_forces(u, v, w, f["dens"], u0, v0, w0, **forces)
    T = u.dtype.type
    Nf = T(u.shape[0] - 2)
    for x, s in ((u, u0), (v, v0), (w, w0)):
        S3.add_source(x, s, DT)
    u, u0, v, v0, w, w0 = u0, u, v0, v, w0, w
    a = ((T(DT) * T(VISC)) * Nf) * Nf
    for b, x, x0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        S3.lin_solve(b, x, x0, a, T(1) + T(6) * a, K)
    out = Q.project_cg(u, v, w, tol, max_iters, m)
    u0, v0, w0 = out["u"], out["v"], out["w"]  # (after the swap: the projected velocity is what advect reads)
    u, v, w = (np.zeros_like(u0) for _ in range(3))
    for b, d, d0 in ((1, u, u0), (2, v, v0), (3, w, w0)):
        if maccormack:
            MC.advect_mc(b, d, d0, u0, v0, w0, T(DT))
        else:
            S3.advect(b, d, d0, u0, v0, w0, DT)
    return Q.project_cg(u, v, w, tol, max_iters, m)


# ---- the pass plan a preconditioned solve really ran ---------------------------------------------------------------
JACOBI_OPS = {"jacobi1": 1, "jacobi2": 2, "jacobi3": 3, "jacobi4": 4}


def traced_plans(path):
    """The schedule trace `path` (SF_TRACE_SCHEDULE) -> [(ctx record, [plan, ...])], one entry per context in the order
    of creation (contexts that were alive one after the other). A plan is what slab 0 ran between two consecutive
    cg_dot ops — one z = M(r) of a preconditioned solve — in the notation of pcg_cases: the sweeps of each pass
    (jacobi1 .. jacobi4), `C` after the first if a zero_z op came before it and `Z` if not, `+e` where the boundary
    launch of the pass (its op on stream bs) was e planes deeper than max(depth of the pass, G).

    The launches of one pass (boundary and interior, or low, high and interior) have one name and write one buffer; the
    next pass writes the other buffer of the ping-pong, so a change of either starts a new pass.

    Read from the trace: the names, the buffers and the planes the boundary launch wrote. Not read from it: the depth
    that counts as no growth, max(s, G) with a pair four planes deep on G >= 3 (for_planes and pair_depth of
    sf_solver.hpp), which is the formula pcg_cases.model has too — the `+e` is independent of the model in the planes
    written only."""
    out = []
    window = None
    with open(path) as fh:
        for line in fh:
            rec = json.loads(line)
            if rec["t"] == "ctx":
                out.append((rec, []))
                window = None
                continue
            if rec["t"] != "op" or rec["slab"] != 0 or not out:
                continue
            if rec["name"] == "cg_dot":
                if window is not None:
                    out[-1][1].append(_plan_of(window, out[-1][0]["G"]))
                window = []
            elif window is not None and (rec["name"] in JACOBI_OPS or rec["name"] == "zero_z"):
                window.append(rec)
    return out


def slab0_ops(path):
    """The op records of slab 0 in the schedule trace `path`, in order (every op is flushed when it is issued, so the
    trace of a live context can be read between two calls; a last line still being written is left out)."""
    with open(path) as fh:
        text = fh.read()
    recs = [json.loads(line) for line in text[:text.rfind("\n") + 1].splitlines()]
    return [r for r in recs if r["t"] == "op" and r["slab"] == 0]


def passes_of_M(ops, zbufs=None):
    """Of a stretch of slab0_ops on ONE slab (P = 1: one launch per pass): how many passes of z = M(r) it holds, and
    the buffer z was in at its last r.z sum. The buffers of z and its partner are the ones cg_dot reads z from (its
    second access); only the passes of M write them. zbufs: both buffers, where the stretch cannot show them (an M of an
    even number of passes ends in the same one every time)."""
    zbufs = zbufs or {op["acc"][1][1] for op in ops if op["name"] == "cg_dot"}
    writes = [a[1] for op in ops if op["name"] in JACOBI_OPS for a in op["acc"] if a[0] == "w"]
    last = [op["acc"][1][1] for op in ops if op["name"] == "cg_dot"]
    return sum(b in zbufs for b in writes), zbufs, (last[-1] if last else None)


def _plan_of(ops, G):
    passes, zeroed = [], False  # [sweeps, written buffers, boundary depth or None]
    for op in ops:
        if op["name"] == "zero_z":
            zeroed = True
            continue
        s = JACOBI_OPS[op["name"]]
        writes = [a for a in op["acc"] if a[0] == "w"]
        bufs = {a[1] for a in writes}
        if not passes or passes[-1][0] != s or passes[-1][1] != bufs:
            passes.append([s, bufs, None])
        if op["stream"] == "bs":  # slab 0 is a wall slab: its low boundary launch writes planes [G - 1, G + depth)
            passes[-1][2] = writes[0][3] - G
    toks = []
    for n, (s, _, depth) in enumerate(passes):
        nominal = max((4 if G >= 3 else 2) if s == 2 else s, G)
        first = ("C" if zeroed else "Z") if n == 0 else ""
        toks.append(f"{s}{first}" + (f"+{depth - nominal}" if depth is not None and depth != nominal else ""))
    return " ".join(toks)


# ---- kernel forms (a test module that uses a fixture imports its name) ---------------------------------------------
@pytest.fixture(params=["auto", "marching"])
def march_mode(request, monkeypatch):
    """The k-marching S-sweep kernel only takes grids of a few million cells by default (smaller ones do not fill the
    chip with its 512-thread workgroups); "marching" lowers that threshold to zero so that the small, wall-dominated,
    odd-sized cases of these tests run through it as well."""
    if request.param == "marching":
        monkeypatch.setenv("SF_MARCH_MINCELLS_K", "0")
    return request.param


@pytest.fixture(params=["default", "gather", "row", "pairs"])
def advect_form(request, monkeypatch):
    """The cell-to-lane form of advect and of the MacCormack second pass (SF_ADVECT_ROW, read when a context is
    created): four cells per thread with per-cell gathers of (i0, i0+1) pairs; one cell per lane with the i0+1 samples
    taken from the neighbour lane; one cell per lane with own pair loads. Unset = the default (the second / third serve
    the three velocity components in fp32 / fp64 and the first everything else); 0 / 2 / 3 force one form for every
    call, so each sees every size, dtype and boundary mode, for one field and for three. Used directly (all four
    forms) or through indirect parametrisation. (A fourth form — two cells per lane, aligned pair gathers, 32-bit
    buffer offsets — was built in round 3, bit-identical and not faster: profiles/r03_advect_two_cells_experiment.txt.)"""
    form = request.param
    if form != "default":
        monkeypatch.setenv("SF_ADVECT_ROW", {"gather": "0", "row": "2", "pairs": "3"}[form])
    else:
        monkeypatch.delenv("SF_ADVECT_ROW", raising=False)
    return form
