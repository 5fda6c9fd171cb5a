"""Volume rendering and light marching on the GPU (docs/SPEC.md §12): sf_render, sf_render_read and sf_light through
libsfgpu.so against the numpy reference (tests/render_ref.py) on the cases of tests/render_cases.py. Every comparison is
exact equality of the bits (in the special-value family a NaN equals any NaN: its payload is unspecified), on every
axis and direction, in both precisions, at every size, for every decomposition and transport."""
import os
import subprocess

import numpy as np
import pytest

import render_cases as RC
import render_ref as RR
import schedule_check as SCK
import stable_ref as S3
from gpu_support import DT, ROOT, S, assert_same_bits, bench_state, check_transport, make, upload_all

pytestmark = pytest.mark.gpu
DTYPE_IDS = ["f32", "f64"]
SHAPES = [(N, dt) for N in RC.SIZES for dt in RC.DTYPES]
SHAPE_IDS = [f"N{N}-{RC.dname(dt)}" for N, dt in SHAPES]


def check_view(fs, dens, emit, sigma, axis, high, what, nan_ok=False, family=None):
    """render with emit (slot user0), without, and with emit == dens, and light (into user1), against the reference; and
    §12.1: render's Tr is light's value at the last cell visited times (1 - a) of that cell."""
    N = dens.shape[0] - 2
    for slot, e, tag in (("user0", emit, "emit"), (None, None, "no emit"), ("dens", dens, "emit == dens")):
        C, Tr = fs.render("dens", slot, axis, high, sigma)
        wC, wTr = RR.render(dens, e, axis, high, sigma)
        if family is not None and e is not dens:
            RC.check_conditions(family, N, dens, wC, wTr)
        assert_same_bits(C, wC, f"{what}: C ({tag})", nan_ok=nan_ok or e is dens)
        assert_same_bits(Tr, wTr, f"{what}: Tr ({tag})")
    fs.light("user1", "dens", axis, high, sigma)
    got = fs.download("user1")
    assert_same_bits(got, RR.light(dens, axis, high, sigma), f"{what}: light")
    last = N if not high else 1
    T = dens.dtype.type
    exit_tr = RR.cells(got, axis, last) * (T(1) - RR.opacity(RR.scalar(N, dens.dtype, sigma), RR.cells(dens, axis, last)))
    assert_same_bits(exit_tr.astype(dens.dtype), Tr, f"{what}: light's exit value times (1 - a)")


@pytest.mark.parametrize("N,dtype", SHAPES, ids=SHAPE_IDS)
def test_every_view_at_every_size(N, dtype):
    with make(N, dtype) as fs:
        for family in RC.FAMILIES:
            dens, emit, sigma = RC.inputs(family, N, dtype)
            fs.upload("dens", dens)
            fs.upload("user0", emit)
            for (axis, high), vid in zip(RC.VIEWS, RC.VIEW_IDS):
                check_view(fs, dens, emit, sigma, axis, high, f"{family} N={N} {vid}", nan_ok=family == "special",
                           family=family)
            assert_same_bits(fs.download("dens"), dens, "dens after the calls")
            assert_same_bits(fs.download("user0"), emit, "emit after the calls")


@pytest.mark.parametrize("N,dtype", SHAPES, ids=SHAPE_IDS)
def test_closed_forms(N, dtype):
    """§12.1 through the library: zero density, s * d = 0.5 exactly, an opaque first cell."""
    T = np.dtype(dtype).type
    mant = np.finfo(dtype).nmant + 1
    with make(N, dtype) as fs:
        for (axis, high), vid in zip(RC.VIEWS, RC.VIEW_IDS):
            for kind in ("zero", "half", "opaque"):
                dens, emit, sigma = RC.closed(kind, N, dtype, axis, high)
                fs.upload("dens", dens)
                fs.upload("user0", emit)
                check_view(fs, dens, emit, sigma, axis, high, f"{kind} N={N} {vid}")
                C, Tr = fs.render("dens", None if kind != "opaque" else "user0", axis, high, sigma)
                if kind == "zero":
                    assert_same_bits(C, np.zeros((N, N), dtype), "zero density: C = +0")
                    assert_same_bits(Tr, np.ones((N, N), dtype), "zero density: Tr = 1")
                elif kind == "half" and N <= mant:
                    assert_same_bits(Tr, np.full((N, N), T(2.0) ** -N, dtype), "half: Tr = 2^-N")
                    assert_same_bits(C, np.full((N, N), T(1) - T(2.0) ** -N, dtype), "half: C = 1 - 2^-N")
                elif kind == "opaque":
                    assert_same_bits(Tr, np.zeros((N, N), dtype), "opaque first cell: Tr = +0")
                    assert_same_bits(C, np.ascontiguousarray(RR.cells(emit, axis, N if high else 1)),
                                     "opaque first cell: C = e of that cell")


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N,P,transport", RC.DECOMPOSED, ids=[f"N{n}-P{p}-{t}" for n, p, t in RC.DECOMPOSED])
def test_every_view_on_every_decomposition(N, P, transport, dtype):
    """The k-axis chain in both directions, and the i and j views slab by slab. After light, dst's ghost planes are
    current: one advect that reads it equals the reference's."""
    rng = np.random.RandomState(40 + N)
    u, v, w = ((0.2 / (DT * N) * rng.standard_normal((N + 2,) * 3)).astype(dtype) for _ in range(3))
    with make(N, dtype, P=P, transport=transport) as fs:
        g0 = fs.transport_info()["rccl_groups"]
        for n, a in (("u", u), ("v", v), ("w", w)):
            fs.upload(n, a)
        for family in RC.FAMILIES:
            dens, emit, sigma = RC.inputs(family, N, dtype)
            fs.upload("dens", dens)
            fs.upload("user0", emit)
            for (axis, high), vid in zip(RC.VIEWS, RC.VIEW_IDS):
                what = f"{family} N={N} P={P} {transport} {vid}"
                check_view(fs, dens, emit, sigma, axis, high, what, nan_ok=family == "special", family=family)
                if axis == 2 and family == "random":
                    C, Tr = fs.render("dens", "user0", axis, high, sigma)
                    kC, kTr = RR.render_slabs(dens, emit, high, sigma, P)
                    assert_same_bits(C, kC, f"{what}: C of the chain of {P} slabs")
                    assert_same_bits(Tr, kTr, f"{what}: Tr of the chain of {P} slabs")
                if family == "random" and (axis == 2 or high == axis):
                    fs.light("user1", "dens", axis, high, sigma)
                    fs.advect(0, "user2", "user1", "u", "v", "w")
                    fs.sync()
                    want = np.zeros_like(dens)
                    S3.advect(0, want, RR.light(dens, axis, high, sigma), u, v, w, DT)
                    assert_same_bits(fs.download("user2"), want, f"{what}: advect of the light field")
        check_transport(fs, transport, P)
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > g0
        else:
            assert fs.transport_info()["rccl_groups"] == g0


def step_ops(path):
    """Per context of a schedule trace: its records that are not those of a render or a light march, without buffer
    ids (a context that renders has allocated more buffers)."""
    out = []
    with open(path) as fh:
        for c in SCK.split_contexts(fh.readlines()):
            recs = []
            for r in c["records"]:
                name = r.get("name", "")
                if name.startswith(("render", "light", "rays_")):
                    continue
                r = {k: v for k, v in r.items() if k != "_line"}
                if "acc" in r:
                    r["acc"] = [[a[0], a[2], a[3]] for a in r["acc"]]
                recs.append(r)
            out.append(recs)
    return out


@pytest.mark.parametrize("P,transport,graph", [(1, "copy", False), (1, "copy", True), (4, "copy", False),
                                                (2, "rccl-self", False)])
def test_render_does_not_change_a_step(P, transport, graph, monkeypatch):
    """vel_step + dens_step before and after a render (all three axes, a light march into a free slot) equal the same
    run without it in bits; with SF_GRAPH=1 the render sits between replayed steps. The schedule trace of the steps is
    the same record for record on one slab; on several slabs a render joins the compute streams, so the next step has
    fewer waits to issue, and the light march exchanges its ghost planes: there the launches are compared, op by op."""
    N, dtype, steps = 32, np.float32, 3
    if graph:
        monkeypatch.setenv("SF_GRAPH", "1")
    rng = np.random.RandomState(21)
    f = {n: (0.1 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in S().FIELD_NAMES}
    for n in ("u", "v", "w"):
        f[n] = (0.05 * rng.standard_normal((N + 2,) * 3)).astype(dtype)
    out = []
    for watch in (False, True):
        with make(N, dtype, P=P, transport=transport) as fs:
            upload_all(fs, f)
            fs.fill("user1", 0.0)  # (a slot allocated between two steps is a new buffer arrangement: a new capture)
            for _ in range(steps):
                fs.vel_step()
                if watch:
                    fs.light("user1", "dens", 2, 1, 3.0)
                    fs.render("dens", "user1", 1, 0, 3.0)
                fs.dens_step()
                if watch:
                    fs.render("dens", None, 0, 1, 3.0)
                    fs.render("dens", "dens", 2, 0, 3.0)
            fs.sync()
            out.append({n: fs.download(n) for n in S().FIELD_NAMES})
    for n in S().FIELD_NAMES:
        assert_same_bits(out[1][n], out[0][n], f"{n} with and without render calls")
    trace = os.environ["SF_TRACE_SCHEDULE"]
    plain, watched = step_ops(trace)[-2:]
    if P == 1:
        assert watched == plain, "the steps of a run that renders issue other launches"
    else:  # (the light march publishes its ghost planes: an exchange of its own)
        ops = lambda recs: [(r["name"], r["slab"], r["stream"], r["acc"]) for r in recs
                            if r["t"] == "op" and not r["name"].startswith("halo")]
        assert ops(watched) == ops(plain), "the steps of a run that renders issue other launches"


def test_error_returns():
    N = 8
    L = S().lib
    with make(N, np.float32) as fs:
        img = np.zeros((N, N), np.float32)
        ptr = img.ctypes.data
        assert L.sf_render_read(fs._h, ptr, ptr) == S().SF_ERR_INVALID  # a read before any render
        assert L.sf_render(fs._h, None) == S().SF_ERR_INVALID
        good = dict(dens="dens", emit=None, axis=0, from_high=0, sigma=1.0)
        for bad in (dict(axis=-1), dict(axis=3), dict(from_high=2), dict(from_high=-1), dict(sigma=-1.0),
                    dict(sigma=float("nan")), dict(sigma=float("inf")), dict(dens=12), dict(dens=-1), dict(emit=12),
                    dict(emit=-2)):
            with pytest.raises(S().SfError) as e:
                fs.render(**{**good, **bad})
            assert e.value.status == S().SF_ERR_INVALID, bad
        assert L.sf_render_read(fs._h, ptr, ptr) == S().SF_ERR_INVALID  # none of them counted as a render
        for bad in ((6, 6, 0, 0, 1.0), (12, 6, 0, 0, 1.0), (8, -1, 0, 0, 1.0), (8, 6, 3, 0, 1.0), (8, 6, 0, 2, 1.0),
                    (8, 6, 0, 0, -0.5), (8, 6, 0, 0, float("nan"))):
            assert L.sf_light(fs._h, *bad) == S().SF_ERR_INVALID, bad
        C, Tr = fs.render("user2", "user3", 1, 1, 2.0)  # unused slots: allocated as zeros first
        assert_same_bits(C, np.zeros((N, N), np.float32), "C of a zero field")
        assert_same_bits(Tr, np.ones((N, N), np.float32), "Tr of a zero field")
        assert L.sf_render_read(fs._h, None, None) == S().SF_OK  # either pointer may be NULL
        assert L.sf_render_read(fs._h, None, ptr) == S().SF_OK
        assert_same_bits(img, Tr, "Tr alone")
    assert L.sf_render(None, None) == S().SF_ERR_INVALID
    assert L.sf_light(None, 8, 6, 0, 0, 1.0) == S().SF_ERR_INVALID


def test_driver_writes_the_rendered_frames(tmp_path):
    """sf_driver --n 16 --steps 2 --every 1 --render j+:4:k-: the bytes of render_0000.pgm and render_0001.pgm are the
    numpy quantisation of the reference's image of the same run's density, lit from the high k side."""
    N, K = 16, 20
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    run = subprocess.run([exe, "--n", str(N), "--steps", "2", "--every", "1", "--quiet", "--out", str(tmp_path),
                          "--render", "j+:4:k-"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    f, src = bench_state(N, np.float32)
    with make(N, np.float32, K=K) as fs:
        upload_all(fs, f)
        for n, a in src.items():
            fs.upload({"u0": "user0", "v0": "user1", "w0": "user2", "dens0": "user3"}[n], a)
        fs.bind_sources()
        for frame in range(2):
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            dens = fs.download("dens")
            C, _ = RR.render(dens, RR.light(dens, 2, 1, 4.0), 1, 0, 4.0)
            got = open(tmp_path / f"render_{frame:04d}.pgm", "rb").read()
            assert got == RR.pgm_bytes(C), f"render_{frame:04d}.pgm"
            assert C.max() > 0.01  # (an image of something)
