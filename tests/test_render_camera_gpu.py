"""Perspective volume rendering on the GPU (docs/SPEC.md §14): sf_render_camera, sf_camera_passes_get and sf_camera_frame
through libsfgpu.so against the numpy reference (tests/render_camera_ref.py) on the cases of tests/camera_cases.py.
Every comparison is exact equality of the bits on both images (in the special-value family a NaN of C equals any NaN: its
payload is unspecified), for every size, dtype, camera, step, image, decomposition and transport. One context holds
every slab of a decomposition here, so the image is read from the slab the last pass ended on and must be the whole
image; that a context without that slab reads back zeros needs several ranks and is held on the reference only
(render_camera_ref.held_pixels, tests/test_render_camera_ref.py)."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import render_camera_ref as CR
import render_cases as RC
import render_ref as RR
import render_view_ref as VR
import schedule_check
import view_cases as VC
from gpu_support import ROOT, S, assert_same_bits, bench_state, check_transport, make, random_fields, upload_all

pytestmark = pytest.mark.gpu
DTYPE_IDS = ["f32", "f64"]
SHAPES = [(N, dt) for N in CC.ALL_SIZES for dt in CC.DTYPES]
SHAPE_IDS = [f"N{N}-{CC.dname(dt)}" for N, dt in SHAPES]
PASSES = {CR.UP: "up", CR.DOWN: "down", CR.BOTH: "both"}


def vec(v):
    return (C.c_double * 3)(*map(float, v))


def params(fr):
    """The SfCameraParams of a reference frame."""
    p = S().SfCameraParams()
    for name, v in (("origin", fr.origin), ("du", fr.du), ("dv", fr.dv), ("step", fr.step)):
        setattr(p.view, name, vec(v))
    p.step_du, p.step_dv = vec(fr.step_du), vec(fr.step_dv)
    p.view.width, p.view.height, p.view.samples, p.view.sigma = fr.width, fr.height, fr.samples, float(fr.sigma)
    return p


def view_params(fr):
    """The SfViewParams of a §13 frame."""
    p = S().SfViewParams()
    for name, v in (("origin", fr.origin), ("du", fr.du), ("dv", fr.dv), ("step", fr.step)):
        setattr(p, name, vec(v))
    p.width, p.height, p.samples, p.sigma = fr.width, fr.height, fr.samples, float(fr.sigma)
    return p


def check(fs, fr, emit, want, what, nan_ok=False):
    Cg, Tr = fs.render_camera(params(fr), "dens", "user0" if emit else None)
    assert_same_bits(Cg, np.ascontiguousarray(want[0]), f"{what}: C", nan_ok=nan_ok)
    assert_same_bits(Tr, np.ascontiguousarray(want[1]), f"{what}: Tr")


# ---- 1. every case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", SHAPES, ids=SHAPE_IDS)
def test_every_case(N, dtype):
    with make(N, dtype) as fs:
        loaded = None
        for c in sorted(CC.cases_of(N, dtype), key=lambda c: c.family):
            dens, emit, _ = CC.inputs(c.family, N, dtype)
            if loaded != c.family:
                if loaded is not None:
                    assert_same_bits(fs.download("dens"), before[0], "dens after the calls")
                    assert_same_bits(fs.download("user0"), before[1], "emit after the calls")
                fs.upload("dens", dens)
                fs.upload("user0", emit)
                loaded, before = c.family, (dens, emit)
            want = CC.reference(c)
            CC.check_conditions(c, *want)
            check(fs, CC.case_frame(c), c.emit, want, CC.case_id(c), nan_ok=c.family == "special")
        assert_same_bits(fs.download("dens"), before[0], "dens after the calls")
        assert_same_bits(fs.download("user0"), before[1], "emit after the calls")


# ---- 2. the frame and the passes of the library --------------------------------------------------------------------
def test_the_frame_of_the_library_renders_the_same():
    """FluidSolver.camera_frame (sf_camera_frame, the tangent taken in Python) instead of the numpy camera."""
    N, dtype, image, step = 13, np.float32, CC.big_image(13), 0.5
    dens, emit, sigma = CC.inputs("random", N, dtype)
    with make(N, dtype) as fs:
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        for cam in ("A", "U", "D"):
            eye, target, up, tan = CC.camera(N, cam)
            fov = float(np.degrees(2.0 * np.arctan(tan)))
            f = fs.camera_frame(eye, target, up, fov, image[0], image[1], step, sigma)
            # the reference's frame for the tangent the wrapper takes (the case's own up to the rounding of tan(atan(.)))
            fr = CR.camera_frame(N, eye, target, up, math.tan(math.radians(fov) / 2.0), image[0], image[1], step, sigma)
            for got, want in ((f.view.origin, fr.origin), (f.view.du, fr.du), (f.view.dv, fr.dv), (f.view.step, fr.step),
                              (f.step_du, fr.step_du), (f.step_dv, fr.step_dv)):
                assert np.array(got[:]).tobytes() == np.asarray(want, np.float64).tobytes()
            assert (f.view.samples, f.view.sigma, f.view.width, f.view.height) == (fr.samples, sigma, image[0], image[1])
            near = CC.frame(N, cam, step, image)
            assert fr.samples == near.samples and np.allclose(fr.step_dv, near.step_dv, rtol=1e-12, atol=0)
            Cg, Tr = fs.render_camera(f, "dens", "user0")
            assert Cg.shape == (image[1], image[0])
            want = CR.render_camera(dens, emit, fr)
            assert_same_bits(Cg, want[0], f"camera {cam}: C")
            assert_same_bits(Tr, want[1], f"camera {cam}: Tr")
            assert fs.camera_passes(f) == PASSES[CR.passes(fr, dtype)] == {"A": "both", "U": "up", "D": "down"}[cam]


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=DTYPE_IDS)
def test_camera_passes(dtype):
    """sf_camera_passes_get is the corner rule of the reference; rays that stay level (r_z = +0) count as up."""
    with make(13, dtype) as fs:
        for N in (13, 34, 70):
            for cam in CC.CAMERAS:
                for image in (CC.big_image(N), CC.CHAIN_VIEW[1], (65, 3)):
                    fr = CC.frame(N, cam, 0.5, image)
                    assert fs.camera_passes(params(fr)) == PASSES[CR.passes(fr, dtype)], (N, cam, image)
            level = CR.of_view(VC.frame(N, 2, *VC.CHAIN_VIEW), VC.SIGMA)
            assert not CR.direction(level, dtype)[2].any()
            assert fs.camera_passes(params(level)) == "up"


# ---- 3. identities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", SHAPES, ids=SHAPE_IDS)
def test_identities(N, dtype):
    """§14.1: with step_du = step_dv = 0 the six frames through the cell centres equal sf_render and sf_render_view
    (|r| = 1); every second cell centre with sigma equals sf_render_view with 2 sigma; edge_frame equals §13's; a zero
    density gives (+0, 1) in every pixel of every camera."""
    dens, emit, sigma = CC.inputs("random", N, dtype)
    with make(N, dtype) as fs:
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        for (axis, high), vid in zip(RC.VIEWS, RC.VIEW_IDS):
            fr = VR.axis_frame(N, axis, high, sigma)
            for e in (True, False):
                what = f"N={N} {vid} emit={e}"
                check(fs, CR.of_view(fr), e, RR.render(dens, emit if e else None, axis, high, sigma), what)
                check(fs, CR.of_view(fr), e, fs.render("dens", "user0" if e else None, axis, high, sigma), f"{what} against sf_render")
                check(fs, CR.of_view(fr), e, fs.render_view(view_params(fr), "dens", "user0" if e else None),
                      f"{what} against sf_render_view")
            two = VR.axis_frame(N, axis, high, 2 * sigma)
            two = two._replace(step=two.step * 2.0, samples=max(N // 2, 1))
            check(fs, CR.of_view(two, sigma), True, fs.render_view(view_params(two), "dens", "user0"), f"N={N} {vid} two cells a step")
        dens, emit, _ = CC.inputs("shells", N, dtype)
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        fr = VC.edge_frame(N)
        check(fs, CR.of_view(fr), True, VR.render_view(dens, emit, fr), f"N={N} edge frame")
        check(fs, CR.of_view(fr), True, fs.render_view(view_params(fr), "dens", "user0"), f"N={N} edge frame against sf_render_view")
        fs.upload("dens", np.zeros_like(dens))
        for cam in CC.CAMERAS:
            fr = CC.frame(N, cam, 0.5, (9, 17))
            check(fs, fr, True, VR.start(fr, dtype), f"N={N} camera {cam} zero density")


# ---- 4. decomposed -------------------------------------------------------------------------------------------------
def crossing(N, dtype, fr, P):
    many = CR.slabs_crossed(N, dtype, fr, P) >= 2
    down = CR.is_down(fr, np.dtype(dtype).type)
    return int(np.count_nonzero(many & ~down)), int(np.count_nonzero(many & down))


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N,P,transport", CC.DECOMPOSED, ids=[f"N{n}-P{p}-{t}" for n, p, t in CC.DECOMPOSED])
def test_every_decomposition(N, P, transport, dtype):
    """Both passes, either pass alone and rays within a slab, on slabs of one plane too (34 / 17): the image equals the
    undecomposed reference."""
    with make(N, dtype, P=P, transport=transport) as fs:
        g0 = fs.transport_info()["rccl_groups"]
        dens, emit, _ = CC.inputs("random", N, dtype)
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        ups = downs = 0
        for cam in CC.CHAIN_CAMERAS:
            fr = CC.frame(N, cam, *CC.CHAIN_VIEW)
            assert fs.camera_passes(params(fr)) == PASSES[CR.passes(fr, dtype)]
            if cam in ("A", "C"):
                u, d = crossing(N, dtype, fr, P)
                print(f"N={N} P={P} camera {cam}: {u} up pixels and {d} down pixels cross a slab boundary")
                ups, downs = ups + u, downs + d
            for e in (True, False):
                check(fs, fr, e, CR.render_camera(dens, emit if e else None, fr), f"N={N} P={P} camera {cam} emit={e}")
        assert ups >= 8 and downs >= 8, (ups, downs)
        level = CR.of_view(VC.frame(N, 2, *VC.CHAIN_VIEW), VC.SIGMA)
        check(fs, level, True, CR.render_camera(dens, emit, level), f"N={N} P={P} level rays")
        for axis, high in ((2, 0), (2, 1)):
            check(fs, CR.of_view(VR.axis_frame(N, axis, high, RC.SIGMA)), True, RR.render(dens, emit, axis, high, RC.SIGMA),
                  f"N={N} P={P} axis {axis} high {high}")
        dens, emit, _ = CC.inputs("special", N, dtype)
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        fr = CC.frame(N, "C", *CC.CHAIN_VIEW)
        check(fs, fr, True, CR.render_camera(dens, emit, fr), f"N={N} P={P} special", nan_ok=True)
        check_transport(fs, transport, P)
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > g0
        else:
            assert fs.transport_info()["rccl_groups"] == g0


def test_the_schedule_of_a_mixed_frame_is_clean():
    """The trace of a mixed frame on rccl-self (SF_TRACE_SCHEDULE, set for every GPU test): the stage that resumes reads
    and writes the pair of its slab, the ops carry their pass in the name, and schedule_check finds nothing to object
    to."""
    N, P, dtype = 34, 2, np.float32
    trace = os.environ["SF_TRACE_SCHEDULE"]
    dens, emit, _ = CC.inputs("random", N, dtype)
    fr = CC.frame(N, "A", *CC.CHAIN_VIEW)
    with make(N, dtype, P=P, transport="rccl-self") as fs:
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        check(fs, fr, True, CR.render_camera(dens, emit, fr), "mixed frame, emit")
        check(fs, fr, False, CR.render_camera(dens, None, fr), "mixed frame, plain")
        check(fs, CC.frame(N, "U", *CC.CHAIN_VIEW), False, CR.render_camera(dens, None, CC.frame(N, "U", *CC.CHAIN_VIEW)), "up frame")
    ops = [json.loads(line) for line in open(trace)]
    ops = [r for r in ops if r["t"] == "op" and r["name"].startswith("render_camera")]
    names = [(r["name"], r["slab"]) for r in ops]
    assert names == [("render_camera_emit_up", 0), ("render_camera_emit_up", 1), ("render_camera_emit_down", 1),
                     ("render_camera_emit_down", 0), ("render_camera_up", 0), ("render_camera_up", 1),
                     ("render_camera_down", 1), ("render_camera_down", 0), ("render_camera_both", 0),
                     ("render_camera_both", 1)], names
    resumed = ops[2]  # the first stage of the downward pass: a read and a write of one buffer
    written = {a[1] for a in resumed["acc"] if a[0] == "w"}
    read = {a[1] for a in resumed["acc"] if a[0] == "r"}
    assert len(written) == 1 and written <= read, resumed
    first = ops[0]  # the first stage of the upward pass starts from nothing: it reads no pair
    assert not ({a[1] for a in first["acc"] if a[0] == "w"} & {a[1] for a in first["acc"] if a[0] == "r"}), first
    ctxs, bad = schedule_check.check_file(trace)
    assert len(ctxs) >= 1 and not bad, "launch schedule hazard:\n" + schedule_check.describe(bad)


def test_loopback_context_renders_its_own_planes():
    """A loopback context stands for one rank of several and has nobody to receive a pair from: a mixed frame returns
    SF_OK (its image, of its own planes only, means nothing; a zero density gives (+0, 1) whatever is marched)."""
    N, nranks, rank = 32, 4, 1
    fr = CC.frame(N, "A", 0.5, (9, 17))
    with S().FluidSolver(N, dtype="f32", iters=4, rank=rank, nranks=nranks, flags=S().SF_FLAG_LOOPBACK_HALO) as fs:
        p = params(fr)
        p.view.dens, p.view.emit = S().FIELD_IDS["dens"], -1
        assert S().lib.sf_render_camera(fs._h, C.byref(p)) == S().SF_OK
        img = np.full((fr.height, fr.width), 7, np.float32)
        tr = np.zeros((fr.height, fr.width), np.float32)
        assert S().lib.sf_render_view_read(fs._h, img.ctypes.data, tr.ctypes.data) == S().SF_OK
        assert_same_bits(img, np.zeros_like(img), "C of a zero density")
        assert_same_bits(tr, np.ones_like(tr), "Tr of a zero density")


# ---- 5. interleaving -----------------------------------------------------------------------------------------------
def test_the_view_read_returns_the_last_image_of_either_call():
    N, dtype = 34, np.float32
    dens, emit, sigma = CC.inputs("random", N, dtype)
    L = S().lib
    with make(N, dtype, P=2) as fs:
        fs.upload("dens", dens)
        fs.upload("user0", emit)
        rp = S().SfRenderParams(axis=2, from_high=1, sigma=sigma, dens=S().FIELD_IDS["dens"], emit=S().FIELD_IDS["user0"])
        assert L.sf_render(fs._h, C.byref(rp)) == S().SF_OK
        vfr = VC.frame(N, 0, 1.0, (9, 17))
        vp = view_params(vfr)
        vp.dens, vp.emit = S().FIELD_IDS["dens"], S().FIELD_IDS["user0"]
        assert L.sf_render_view(fs._h, C.byref(vp)) == S().SF_OK
        cfr = CC.frame(N, "A", 0.5, CC.big_image(N))  # another size: the pair is allocated afresh
        cp = params(cfr)
        cp.view.dens, cp.view.emit = S().FIELD_IDS["dens"], S().FIELD_IDS["user0"]
        assert L.sf_render_camera(fs._h, C.byref(cp)) == S().SF_OK
        Cg, Tr = np.zeros((cfr.height, cfr.width), dtype), np.zeros((cfr.height, cfr.width), dtype)
        assert L.sf_render_view_read(fs._h, Cg.ctypes.data, Tr.ctypes.data) == S().SF_OK
        want = CR.render_camera(dens, emit, cfr)
        assert_same_bits(Cg, want[0], "the camera's C through sf_render_view_read")
        assert_same_bits(Tr, want[1], "the camera's Tr through sf_render_view_read")
        Ca, Ta = np.zeros((N, N), dtype), np.zeros((N, N), dtype)
        assert L.sf_render_read(fs._h, Ca.ctypes.data, Ta.ctypes.data) == S().SF_OK
        wC, wTr = RR.render(dens, emit, 2, 1, sigma)
        assert_same_bits(Ca, wC, "sf_render's C after a camera render")
        assert_same_bits(Ta, wTr, "sf_render's Tr after a camera render")
        got = fs.render_view(view_params(vfr), "dens", "user0")  # and a view render afterwards behaves as before
        want = VR.render_view(dens, emit, vfr)
        assert_same_bits(got[0], want[0], "the view's C after a camera render")
        assert_same_bits(got[1], want[1], "the view's Tr after a camera render")
        for fr in (CC.frame(N, "D", 1.7, (8, 8)), CC.frame(N, "C", 1.0, (65, 3)), CC.frame(N, "U", 0.5, (9, 17))):
            check(fs, fr, True, CR.render_camera(dens, emit, fr), "a pair of another size")


@pytest.mark.parametrize("P,transport,graph", [(1, "copy", False), (1, "copy", True), (4, "copy", False),
                                                (2, "rccl-self", False)])
def test_render_camera_does_not_change_a_step(P, transport, graph, monkeypatch):
    """vel_step + dens_step with camera renders in between equal the same run without them in bits, fields included;
    with SF_GRAPH=1 the renders sit between replayed steps. A Jacobi solve before and after a render likewise."""
    N, dtype, steps = 32, np.float32, 3
    if graph:
        monkeypatch.setenv("SF_GRAPH", "1")
    f = random_fields(N, dtype, 29)
    frames = [CC.frame(N, "A", 0.5, (9, 17)), CC.frame(N, "D", 1.0, (33, 8))]
    out = []
    for watch in (False, True):
        with make(N, dtype, P=P, transport=transport) as fs:
            upload_all(fs, f)
            for _ in range(steps):
                fs.vel_step()
                if watch:
                    fs.render_camera(params(frames[0]), "dens", "u")
                fs.dens_step()
                if watch:
                    fs.sync()
                    dens = fs.download("dens")
                    check(fs, frames[1], False, CR.render_camera(dens, None, frames[1]), "the camera image of the step's density")
            fs.lin_solve(0, "dens0", "dens", 0.3, 2.8, 4)
            if watch:
                fs.render_camera(params(frames[0]), "dens0", None)
            fs.lin_solve(0, "dens", "dens0", 0.3, 2.8, 4)
            fs.sync()
            out.append({n: fs.download(n) for n in S().FIELD_NAMES})
    for n in S().FIELD_NAMES:
        assert_same_bits(out[1][n], out[0][n], f"{n} with and without camera renders")


def test_error_returns():
    N = 8
    L = S().lib
    INV = S().SF_ERR_INVALID
    with make(N, np.float32) as fs:
        img = np.zeros((4, 4), np.float32)
        assert L.sf_render_camera(fs._h, None) == INV
        c = (N + 1) / 2.0
        good = fs.camera_frame((c, c - 20, c + 3), (c, c, c), (0, 0, 1), 40.0, 4, 4, 1.0, 2.0)
        nan, inf = float("nan"), float("inf")

        def call(view=None, **bad):
            p = S().SfCameraParams.from_buffer_copy(good)
            p.view.dens, p.view.emit = S().FIELD_IDS["dens"], -1
            for k, v in (view or {}).items():
                if isinstance(v, tuple):
                    getattr(p.view, k)[v[0]] = v[1]
                else:
                    setattr(p.view, k, v)
            for k, v in bad.items():
                getattr(p, k)[v[0]] = v[1]
            return L.sf_render_camera(fs._h, C.byref(p))

        for bad in (dict(step_du=(0, nan)), dict(step_dv=(1, inf)), dict(step_du=(2, 2e38)), dict(view=dict(origin=(0, nan))),
                    dict(view=dict(du=(1, inf))), dict(view=dict(du=(1, 3e38))), dict(view=dict(dv=(2, -inf))),
                    dict(view=dict(step=(0, nan))), dict(view=dict(step=(0, 1e39))), dict(view=dict(sigma=-1.0)),
                    dict(view=dict(sigma=nan)), dict(view=dict(sigma=inf)), dict(view=dict(width=0)),
                    dict(view=dict(width=16385)), dict(view=dict(height=0)), dict(view=dict(height=-1)),
                    dict(view=dict(samples=0)), dict(view=dict(samples=65537)), dict(view=dict(dens=12)),
                    dict(view=dict(dens=-1)), dict(view=dict(emit=12)), dict(view=dict(emit=-2))):
            assert call(**bad) == INV, bad
        assert L.sf_render_view_read(fs._h, img.ctypes.data, None) == INV  # none of them counted as a render
        assert call(view=dict(dens=S().FIELD_IDS["user2"], emit=S().FIELD_IDS["user3"])) == S().SF_OK
        Tr = np.zeros((4, 4), np.float32)
        assert L.sf_render_view_read(fs._h, img.ctypes.data, Tr.ctypes.data) == S().SF_OK
        assert_same_bits(img, np.zeros((4, 4), np.float32), "C of a zero field")
        assert_same_bits(Tr, np.ones((4, 4), np.float32), "Tr of a zero field")
        assert call(view=dict(samples=65536, width=1, height=1)) == S().SF_OK
    with make(N, np.float64) as fs:  # finite in fp64: the same doubles pass
        p = S().SfCameraParams.from_buffer_copy(good)
        p.view.dens, p.view.emit = S().FIELD_IDS["dens"], -1
        p.step_du[2] = 2e38
        assert L.sf_render_camera(fs._h, C.byref(p)) == S().SF_OK
    assert L.sf_render_camera(None, None) == INV


def test_driver_writes_the_camera_frames(tmp_path):
    """sf_driver --n 34 --steps 2 --every 1 --render-camera ...: the bytes of camera_0001.pgm are the numpy quantisation
    of the reference's image of the same run's density."""
    N, K = 34, 20
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    run = subprocess.run([exe, "--n", str(N), "--steps", "2", "--every", "1", "--quiet", "--out", str(tmp_path),
                          "--render-camera", "-20,-5,22:17.5,17.5,17.5:37x34:4:50:0.5"], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr
    f, src = bench_state(N, np.float32)
    fr = CR.camera_frame(N, (-20, -5, 22), (17.5, 17.5, 17.5), (0, 0, 1), math.tan(50.0 * (math.pi / 360.0)), 37, 34, 0.5, 4.0)
    with make(N, np.float32, K=K) as fs:
        upload_all(fs, f)
        for n, a in src.items():
            fs.upload({"u0": "user0", "v0": "user1", "w0": "user2", "dens0": "user3"}[n], a)
        fs.bind_sources()
        for frame in range(2):
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            Cw, _ = CR.render_camera(fs.download("dens"), None, fr)
            got = open(tmp_path / f"camera_{frame:04d}.pgm", "rb").read()
            assert got == RR.pgm_bytes(Cw), f"camera_{frame:04d}.pgm"
        assert Cw.max() > 0.01  # (an image of something)
