"""Orthographic volume rendering from any direction on the GPU (docs/SPEC.md §13): sf_render_view, sf_render_view_read
and sf_view_frame through libsfgpu.so against the numpy reference (tests/render_view_ref.py) on the cases of
tests/view_cases.py. Every comparison is exact equality of the bits on both images (in the special-value family a NaN of
C equals any NaN: its payload is unspecified), for every size, dtype, direction, step, image, decomposition and
transport."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import render_cases as RC
import render_ref as RR
import render_view_ref as VR
import view_cases as VC
from gpu_support import ROOT, S, assert_same_bits, bench_state, check_transport, make, upload_all

pytestmark = pytest.mark.gpu
DTYPE_IDS = ["f32", "f64"]
SHAPES = [(N, dt) for N in VC.SIZES for dt in VC.DTYPES]
SHAPE_IDS = [f"N{N}-{VC.dname(dt)}" for N, dt in SHAPES]


def params(fr):
    """The SfViewParams of a reference frame."""
    p = S().SfViewParams()
    for name, v in (("origin", fr.origin), ("du", fr.du), ("dv", fr.dv), ("step", fr.step)):
        setattr(p, name, (C.c_double * 3)(*map(float, v)))
    p.width, p.height, p.samples, p.sigma = fr.width, fr.height, fr.samples, float(fr.sigma)
    return p


def check(fs, fr, emit, want, what, nan_ok=False):
    Cg, Tr = fs.render_view(params(fr), "dens", "user0" if emit else None)
    assert_same_bits(Cg, np.ascontiguousarray(want[0]), f"{what}: C", nan_ok=nan_ok)
    assert_same_bits(Tr, np.ascontiguousarray(want[1]), f"{what}: Tr")


@pytest.mark.parametrize("direction", range(len(VC.DIRECTIONS)), ids=VC.DIR_IDS)
@pytest.mark.parametrize("N,dtype", SHAPES, ids=SHAPE_IDS)
def test_every_case(N, dtype, direction):
    with make(N, dtype) as fs:
        loaded = None
        for c in VC.cases_of(N, dtype):
            if c.direction != direction:
                continue
            dens, emit, _ = VC.inputs(c.family, N, dtype)
            if loaded != c.family:
                fs.upload("dens", dens)
                fs.upload("user0", emit)
                loaded = c.family
            want = VC.reference(c)
            VC.check_conditions(c, *want)
            check(fs, VC.case_frame(c), c.emit, want, VC.case_id(c), nan_ok=c.family == "special")
        assert_same_bits(fs.download("dens"), dens, "dens after the calls")
        assert_same_bits(fs.download("user0"), emit, "emit after the calls")


def test_the_frame_of_the_library_renders_the_same():
    """FluidSolver.view_frame (sf_view_frame) instead of the numpy camera: the same image."""
    c = VC.Case("random", 13, np.float32, 0, 0.5, VC.big_image(13), True)
    dens, emit, sigma = VC.inputs(c.family, c.N, c.dtype)
    d, up = VC.DIRECTIONS[c.direction]
    with make(c.N, c.dtype) as fs:
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        Cg, Tr = fs.render_view(fs.view_frame(d, up, c.image[0], c.image[1], c.step, sigma), "dens", "user0")
        assert Cg.shape == (c.image[1], c.image[0])
        assert_same_bits(Cg, np.ascontiguousarray(VC.reference(c)[0]), "C")
        assert_same_bits(Tr, np.ascontiguousarray(VC.reference(c)[1]), "Tr")


@pytest.mark.parametrize("N,dtype", SHAPES, ids=SHAPE_IDS)
def test_axis_frames(N, dtype):
    """§13.1: the six frames through the cell centres equal the axis-aligned render of §12 — the reference's and
    sf_render's on the same context — with and without emission. And edge_frame: samples exactly on two faces."""
    dens, emit, sigma = VC.inputs("random", N, dtype)
    with make(N, dtype) as fs:
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        for (axis, high), vid in zip(RC.VIEWS, RC.VIEW_IDS):
            fr = VR.axis_frame(N, axis, high, sigma)
            for e in (True, False):
                want = RR.render(dens, emit if e else None, axis, high, sigma)
                check(fs, fr, e, want, f"N={N} {vid} emit={e}")
                lib = fs.render("dens", "user0" if e else None, axis, high, sigma)
                check(fs, fr, e, lib, f"N={N} {vid} emit={e} against sf_render")
        dens, emit, sigma = VC.inputs("shells", N, dtype)
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        fr = VC.edge_frame(N)
        check(fs, fr, True, VR.render_view(dens, emit, fr), f"N={N} edge frame")


@pytest.mark.parametrize("N,dtype", SHAPES, ids=SHAPE_IDS)
def test_closed_forms(N, dtype):
    """The closed family (§12.1: zero, half, opaque) through the view: on the six axis frames the exact images and
    §12's reference, and one oblique frame each against the reference; a zero density gives (+0, 1) along it."""
    d, step, image = VC.CLOSED_VIEW
    oblique = VC.frame(N, d, step, image)
    with make(N, dtype) as fs:
        for (axis, high), vid in zip(RC.VIEWS, RC.VIEW_IDS):
            fr = VR.axis_frame(N, axis, high, RC.SIGMA)
            for kind in VC.CLOSED_KINDS:
                dens, emit, sigma = VC.closed(kind, N, dtype, axis, high)
                fs.upload("dens", dens)
                fs.upload("user0", emit)
                what = f"{kind} N={N} {vid}"
                check(fs, fr, True, RR.render(dens, emit, axis, high, sigma), what)
                want = VC.closed_expected(kind, N, dtype, emit, axis, high)
                if want is not None:
                    check(fs, fr, True, want, f"{what}: the closed form")
                if kind == "half":
                    check(fs, fr, False, RR.render(dens, None, axis, high, sigma), f"{what} plain")
                    if VC.half_expected(N, dtype) is not None:
                        check(fs, fr, False, VC.half_expected(N, dtype), f"{what}: C = 1 - 2^-N, Tr = 2^-N")
                if (axis, high) == (2, 0):
                    want = VR.render_view(dens, emit, oblique)
                    if kind == "zero":
                        want = VR.start(oblique, dtype)
                    check(fs, oblique, True, want, f"{what}: oblique")


@pytest.mark.parametrize("dtype", VC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N,P,transport", VC.DECOMPOSED, ids=[f"N{n}-P{p}-{t}" for n, p, t in VC.DECOMPOSED])
def test_every_decomposition(N, P, transport, dtype):
    """The chain in both directions and within a slab (step_z = 0), on slabs of one plane too (34 / 17)."""
    with make(N, dtype, P=P, transport=transport) as fs:
        g0 = fs.transport_info()["rccl_groups"]
        dens, emit, _ = VC.inputs("random", N, dtype)
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        for d in range(len(VC.DIRECTIONS)):
            fr = VC.frame(N, d, *VC.CHAIN_VIEW)
            for e in (True, False):
                check(fs, fr, e, VR.render_view(dens, emit if e else None, fr), f"N={N} P={P} {VC.DIR_IDS[d]} emit={e}")
            for c in VC.cases_of(N, dtype):
                if c.direction == d and c.family == "random" and c.image == VC.big_image(N) and c.step == 0.5:
                    check(fs, VC.case_frame(c), c.emit, VC.reference(c), f"P={P} {VC.case_id(c)}")
        for axis, high in ((2, 0), (2, 1), (0, 1)):
            check(fs, VR.axis_frame(N, axis, high, RC.SIGMA), True, RR.render(dens, emit, axis, high, RC.SIGMA),
                  f"N={N} P={P} axis {axis} high {high}")
        dens, emit, _ = VC.inputs("special", N, dtype)
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        fr = VC.frame(N, 1, *VC.CHAIN_VIEW)
        check(fs, fr, True, VR.render_view(dens, emit, fr), f"N={N} P={P} special", nan_ok=True)
        check_transport(fs, transport, P)
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > g0
        else:
            assert fs.transport_info()["rccl_groups"] == g0


def test_loopback_context_renders_its_own_planes():
    """A loopback context stands for one rank of several and has nobody to receive a pair from: the call returns SF_OK
    (its image, of its own planes only, means nothing; a zero density gives the zero image whatever is marched)."""
    N, nranks, rank = 32, 4, 1
    dens, emit, _ = VC.inputs("random", N, np.float32)
    fr = VC.frame(N, 0, 0.5, (9, 17))
    with S().FluidSolver(N, dtype="f32", iters=4, rank=rank, nranks=nranks, flags=S().SF_FLAG_LOOPBACK_HALO) as fs:
        p = params(fr)
        p.dens, p.emit = S().FIELD_IDS["dens"], -1
        assert S().lib.sf_render_view(fs._h, C.byref(p)) == S().SF_OK
        img = np.zeros((fr.height, fr.width), np.float32)
        assert S().lib.sf_render_view_read(fs._h, img.ctypes.data, None) == S().SF_OK
        assert_same_bits(img, np.zeros_like(img), "C of a zero density")


def test_a_view_render_leaves_the_axis_image_alone_and_reallocates():
    N, dtype = 34, np.float32
    dens, emit, sigma = VC.inputs("random", N, dtype)
    L = S().lib
    with make(N, dtype, P=2) as fs:
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        rp = S().SfRenderParams(axis=2, from_high=1, sigma=sigma, dens=S().FIELD_IDS["dens"], emit=S().FIELD_IDS["user0"])
        assert L.sf_render(fs._h, C.byref(rp)) == S().SF_OK
        frames = [VC.frame(N, 0, 1.0, (9, 17)), VC.frame(N, 1, 0.5, VC.big_image(N)), VC.frame(N, 3, 1.7, (8, 8)),
                  VC.frame(N, 0, 1.0, (9, 17))]
        for n, fr in enumerate(frames):  # a pair of another size each time, larger and smaller
            check(fs, fr, True, VR.render_view(dens, emit, fr), f"frame {n}")
        Cg, Tr = np.zeros((N, N), dtype), np.zeros((N, N), dtype)
        assert L.sf_render_read(fs._h, Cg.ctypes.data, Tr.ctypes.data) == S().SF_OK
        wC, wTr = RR.render(dens, emit, 2, 1, sigma)
        assert_same_bits(Cg, wC, "sf_render's C after view renders")
        assert_same_bits(Tr, wTr, "sf_render's Tr after view renders")
        fr = frames[1]
        Cv = np.zeros((fr.height, fr.width), dtype)
        p = params(fr)
        p.dens, p.emit = S().FIELD_IDS["dens"], S().FIELD_IDS["user0"]
        assert L.sf_render_view(fs._h, C.byref(p)) == S().SF_OK
        fs.render("dens", None, 0, 0, sigma)  # ... and an axis render leaves the view's image alone
        assert L.sf_render_view_read(fs._h, Cv.ctypes.data, None) == S().SF_OK
        assert_same_bits(Cv, VR.render_view(dens, emit, fr)[0], "the view's C after an axis render")


@pytest.mark.parametrize("P,transport,graph", [(1, "copy", False), (1, "copy", True), (4, "copy", False),
                                                (2, "rccl-self", False)])
def test_render_view_does_not_change_a_step(P, transport, graph, monkeypatch):
    """vel_step + dens_step with view renders in between equal the same run without them in bits, fields included; with
    SF_GRAPH=1 the renders sit between replayed steps."""
    N, dtype, steps = 32, np.float32, 3
    if graph:
        monkeypatch.setenv("SF_GRAPH", "1")
    rng = np.random.RandomState(23)
    f = {n: (0.1 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in S().FIELD_NAMES}
    for n in ("u", "v", "w"):
        f[n] = (0.05 * rng.standard_normal((N + 2,) * 3)).astype(dtype)
    frames = [VC.frame(N, 0, 0.5, (9, 17)), VC.frame(N, 1, 1.0, (33, 8))]
    out = []
    for watch in (False, True):
        with make(N, dtype, P=P, transport=transport) as fs:
            upload_all(fs, f)
            for _ in range(steps):
                fs.vel_step()
                if watch:
                    fs.render_view(params(frames[0]), "dens", "u")
                fs.dens_step()
                if watch:
                    fs.sync()
                    dens = fs.download("dens")
                    check(fs, frames[1], False, VR.render_view(dens, None, frames[1]), "the view of the step's density")
            fs.sync()
            out.append({n: fs.download(n) for n in S().FIELD_NAMES})
    for n in S().FIELD_NAMES:
        assert_same_bits(out[1][n], out[0][n], f"{n} with and without view renders")


def test_error_returns():
    N = 8
    L = S().lib
    INV = S().SF_ERR_INVALID
    with make(N, np.float32) as fs:
        img = np.zeros((4, 4), np.float32)
        assert L.sf_render_view_read(fs._h, img.ctypes.data, img.ctypes.data) == INV  # a read before any view render
        assert L.sf_render_view(fs._h, None) == INV
        good = fs.view_frame((1, 2, 3), (0, 0, 1), 4, 4, 1.0, 2.0)
        nan, inf = float("nan"), float("inf")

        def call(**bad):
            p = S().SfViewParams.from_buffer_copy(good)
            p.dens, p.emit = S().FIELD_IDS["dens"], -1
            for k, v in bad.items():
                if isinstance(v, tuple):
                    arr = getattr(p, k)
                    arr[v[0]] = v[1]
                else:
                    setattr(p, k, v)
            return L.sf_render_view(fs._h, C.byref(p))

        for bad in (dict(origin=(0, nan)), dict(du=(1, inf)), dict(dv=(2, -inf)), dict(step=(0, nan)), dict(sigma=-1.0),
                    dict(sigma=nan), dict(sigma=inf), dict(width=0), dict(width=16385), dict(height=0), dict(height=-1),
                    dict(height=16385), dict(samples=0), dict(samples=65537), dict(dens=12), dict(dens=-1), dict(emit=12),
                    dict(emit=-2)):
            assert call(**bad) == INV, bad
        assert L.sf_render_view_read(fs._h, img.ctypes.data, None) == INV  # none of them counted as a render
        assert call(dens=S().FIELD_IDS["user2"], emit=S().FIELD_IDS["user3"]) == S().SF_OK  # unused slots: allocated as zeros first
        Tr = np.zeros((4, 4), np.float32)
        assert L.sf_render_view_read(fs._h, None, None) == S().SF_OK  # either pointer may be NULL
        assert L.sf_render_view_read(fs._h, img.ctypes.data, Tr.ctypes.data) == S().SF_OK
        assert_same_bits(img, np.zeros((4, 4), np.float32), "C of a zero field")
        assert_same_bits(Tr, np.ones((4, 4), np.float32), "Tr of a zero field")
        assert call(samples=65536, width=1, height=1) == S().SF_OK
    assert L.sf_render_view(None, None) == INV


def test_driver_writes_the_view_frames(tmp_path):
    """sf_driver --n 34 --steps 2 --every 1 --render-view 1,2,3:37x34:4:0.5: the bytes of view_0001.pgm are the numpy
    quantisation of the reference's image of the same run's density."""
    N, K = 34, 20
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    run = subprocess.run([exe, "--n", str(N), "--steps", "2", "--every", "1", "--quiet", "--out", str(tmp_path),
                          "--render-view", "1,2,3:37x34:4:0.5"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    f, src = bench_state(N, np.float32)
    fr = VR.view_frame(N, (1, 2, 3), (0, 0, 1), 37, 34, 0.5, 4.0)
    with make(N, np.float32, K=K) as fs:
        upload_all(fs, f)
        for n, a in src.items():
            fs.upload({"u0": "user0", "v0": "user1", "w0": "user2", "dens0": "user3"}[n], a)
        fs.bind_sources()
        for frame in range(2):
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            Cw, _ = VR.render_view(fs.download("dens"), None, fr)
            got = open(tmp_path / f"view_{frame:04d}.pgm", "rb").read()
            assert got == RR.pgm_bytes(Cw), f"view_{frame:04d}.pgm"
        assert Cw.max() > 0.01  # (an image of something)
