"""What the GPU suites (tests/test_*_gpu.py) share: the constants of the step, the case table of the single operators,
the context factory, the comparison, the input builders, the checks against the numpy references and the fixtures
that select a kernel form. A test module imports what it needs from here and from the reference modules, never from
another test module. Importing this module needs no GPU and no libsfgpu.so."""
import socket

import numpy as np
import pytest

import diagnostics_ref as D
import oracle_lib as O
import pressure_cg_ref as R
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
