"""CPU side of perspective volume rendering (docs/SPEC.md §14): the three entry points are declared, exported and
wrapped, sf_camera_params agrees between include/sfgpu.h and the ctypes mirror, sf_camera_frame rejects what it must and
equals the numpy camera in bits, sf_camera_passes_get is the corner rule of the reference, and the driver takes
--render-camera before it touches the device. No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np

import camera_cases as CC
import render_camera_ref as CR
from abi_header import ROOT, declared_functions, enum_values, header_text, struct_members

SYMBOLS = ("sf_render_camera", "sf_camera_passes_get", "sf_camera_frame")
EXE = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")


def S():
    from fluidsolvergpu_amd import solver

    return solver


def vec(v):
    return (C.c_double * 3)(*map(float, v))


def c_frame(N, eye, target, up, tan, W, H, step, sigma):
    f = S().SfCameraParams()
    rc = S().lib.sf_camera_frame(N, vec(eye), vec(target), vec(up), tan, W, H, step, sigma, C.byref(f))
    return rc, f


def c_params(fr):
    """The SfCameraParams of a reference frame."""
    p = S().SfCameraParams()
    for name, v in (("origin", fr.origin), ("du", fr.du), ("dv", fr.dv), ("step", fr.step)):
        setattr(p.view, name, vec(v))
    p.step_du, p.step_dv = vec(fr.step_du), vec(fr.step_dv)
    p.view.width, p.view.height, p.view.samples, p.view.sigma = fr.width, fr.height, fr.samples, float(fr.sigma)
    p.view.dens = p.view.emit = -1
    return p


def c_passes(p, dtype):
    out = C.c_int(-7)
    rc = S().lib.sf_camera_passes_get(C.byref(p), S().SF_F32 if dtype is np.float32 else S().SF_F64, C.byref(out))
    return rc, out.value


def test_symbols_declared_exported_and_wrapped():
    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in S().ABI_SYMBOLS
        assert hasattr(S().lib, name), f"libsfgpu.so does not export {name}"
    for method in ("camera_frame", "render_camera", "camera_passes"):
        assert callable(getattr(S().FluidSolver, method))


def test_struct_and_enum_match_the_header():
    assert struct_members(header_text(), "sf_camera_params") == [("view", "sf_view_params"), ("step_du[3]", "double"),
                                                                 ("step_dv[3]", "double")]
    mirror = S().SfCameraParams._fields_
    assert [n for n, _ in mirror] == ["view", "step_du", "step_dv"]
    assert mirror[0][1] is S().SfViewParams and mirror[1][1] is C.c_double * 3 and mirror[2][1] is C.c_double * 3
    assert C.sizeof(S().SfCameraParams) == 176
    assert [getattr(S().SfCameraParams, n).offset for n, _ in mirror] == [0, 128, 152]
    assert enum_values(header_text(), "sf_camera_passes") == {"SF_CAMERA_UP": "0", "SF_CAMERA_DOWN": "1", "SF_CAMERA_BOTH": "2"}
    assert (S().SF_CAMERA_UP, S().SF_CAMERA_DOWN, S().SF_CAMERA_BOTH) == (CR.UP, CR.DOWN, CR.BOTH) == (0, 1, 2)


def test_prototypes():
    text = " ".join(header_text().split())
    assert "int sf_render_camera(sf_ctx* ctx, const sf_camera_params* p);" in text
    assert "int sf_camera_passes_get(const sf_camera_params* p, int dtype, int* passes);" in text
    assert ("int sf_camera_frame(int N, const double eye[3], const double target[3], const double up[3], double tan_half_fov, "
            "int width, int height, double step, double sigma, sf_camera_params* out);") in text


def test_entry_points_reject_null_pointers():
    L, INV = S().lib, S().SF_ERR_INVALID
    p = S().SfCameraParams()
    out = C.c_int()
    assert L.sf_render_camera(None, C.byref(p)) == INV
    assert L.sf_render_camera(None, None) == INV
    e, t, up = vec((4.5, 4.5, -10)), vec((4.5, 4.5, 4.5)), vec((0, 1, 0))
    assert L.sf_camera_frame(8, None, t, up, 0.5, 4, 4, 1.0, 1.0, C.byref(p)) == INV
    assert L.sf_camera_frame(8, e, None, up, 0.5, 4, 4, 1.0, 1.0, C.byref(p)) == INV
    assert L.sf_camera_frame(8, e, t, None, 0.5, 4, 4, 1.0, 1.0, C.byref(p)) == INV
    assert L.sf_camera_frame(8, e, t, up, 0.5, 4, 4, 1.0, 1.0, None) == INV
    assert L.sf_camera_frame(8, e, t, up, 0.5, 4, 4, 1.0, 1.0, C.byref(p)) == S().SF_OK
    assert L.sf_camera_passes_get(None, S().SF_F32, C.byref(out)) == INV
    assert L.sf_camera_passes_get(C.byref(p), S().SF_F32, None) == INV
    assert L.sf_camera_passes_get(C.byref(p), S().SF_F32, C.byref(out)) == S().SF_OK and out.value == S().SF_CAMERA_UP


def test_camera_frame_rejects_what_it_must():
    nan, inf = float("nan"), float("inf")
    c = 4.5
    good = dict(N=8, eye=(c, c, -10.0), target=(c, c, c), up=(0, 1, 0), tan=0.5, W=4, H=5, step=1.0, sigma=1.0)
    assert c_frame(**good)[0] == S().SF_OK
    assert c_frame(**{**good, "sigma": 0.0})[0] == S().SF_OK
    assert c_frame(**{**good, "W": 16384, "H": 1})[0] == S().SF_OK
    rc, f = c_frame(**{**good, "step": (np.sqrt(3.0) * 8) / 65535.5})
    assert rc == S().SF_OK and f.view.samples == 65536
    for bad in (dict(target=good["eye"]), dict(up=(0, 0, 1)), dict(up=(0, 0, -3)), dict(up=(0, 0, 0)), dict(tan=0.0),
                dict(tan=-1.0), dict(tan=nan), dict(tan=inf), dict(step=0.0), dict(step=-1.0), dict(step=nan),
                dict(step=inf), dict(eye=(c, c, 40.0), target=(c, c, 80.0)), dict(step=1e-4), dict(eye=(nan, c, 0)),
                dict(target=(c, inf, c)), dict(up=(0, nan, 0)), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf),
                dict(W=0), dict(H=0), dict(W=16385), dict(H=16385), dict(W=-3), dict(N=0)):
        rc, f = c_frame(**{**good, **bad})
        assert rc == S().SF_ERR_INVALID, bad


def test_camera_frame_equals_the_numpy_camera_in_bits():
    rng = np.random.RandomState(1401)
    n = 0
    for N in (1, 5, 34, 130, 1024):
        cams = [CC.camera(N, name) for name in CC.CAMERAS]
        c = (N + 1) / 2.0
        cams += [(tuple(c + N * rng.uniform(-2, 2, 3)), tuple(c + N * rng.uniform(-0.5, 0.5, 3)), (0, 0, 1), rng.uniform(0.1, 1.5))
                 for _ in range(4)]
        for eye, target, up, tan in cams:
            W, H = (1, 7, 64, 513)[n % 4], (1, 9, 65)[n % 3]
            step, sigma = (0.5, 1.0, 1.7)[n % 3], (0.0, 4.0, 0.3)[(n // 3) % 3]
            n += 1
            fr = CR.camera_frame(N, eye, target, up, tan, W, H, step, sigma)
            rc, f = c_frame(N, eye, target, up, tan, W, H, step, sigma)
            assert (rc == S().SF_OK) == (fr is not None), (N, eye, target)
            if fr is None:
                continue
            for got, want, name in ((f.view.origin, fr.origin, "origin"), (f.view.du, fr.du, "du"), (f.view.dv, fr.dv, "dv"),
                                    (f.view.step, fr.step, "step"), (f.step_du, fr.step_du, "step_du"),
                                    (f.step_dv, fr.step_dv, "step_dv")):
                got = np.array(got[:], np.float64)
                assert got.tobytes() == np.asarray(want, np.float64).tobytes(), (N, eye, name, got, want)
            assert np.float64(f.view.sigma).tobytes() == np.float64(fr.sigma).tobytes()
            assert (f.view.width, f.view.height, f.view.samples, f.view.dens, f.view.emit) == (W, H, fr.samples, -1, -1)
            for dtype in CC.DTYPES:
                assert c_passes(f, dtype) == (S().SF_OK, CR.passes(fr, dtype)), (N, eye, dtype)
    assert n == 50


def test_camera_passes_get_rejects_what_it_must():
    nan, inf = float("nan"), float("inf")
    good = c_params(CC.frame(13, "A", 0.5, (9, 17)))
    assert c_passes(good, np.float32) == (S().SF_OK, CR.BOTH)
    assert c_passes(good, np.float64) == (S().SF_OK, CR.BOTH)
    out = C.c_int(-7)
    for dtype in (-1, 2, 7):
        assert S().lib.sf_camera_passes_get(C.byref(good), dtype, C.byref(out)) == S().SF_ERR_INVALID and out.value == -7

    def call(dtype, view=None, **bad):
        p = S().SfCameraParams.from_buffer_copy(good)
        for k, v in (view or {}).items():
            if isinstance(v, tuple):
                getattr(p.view, k)[v[0]] = v[1]
            else:
                setattr(p.view, k, v)
        for k, v in bad.items():
            getattr(p, k)[v[0]] = v[1]
        return c_passes(p, dtype)

    for dtype in CC.DTYPES:
        for bad in (dict(step_du=(0, nan)), dict(step_dv=(2, inf)), dict(view=dict(step=(1, -inf))), dict(view=dict(origin=(0, nan))),
                    dict(view=dict(du=(1, inf))), dict(view=dict(dv=(2, nan))), dict(view=dict(width=0)),
                    dict(view=dict(height=0)), dict(view=dict(width=16385)), dict(view=dict(height=-1))):
            assert call(dtype, **bad) == (S().SF_ERR_INVALID, -7), bad
    # finite doubles whose corner pixel is not finite in fp32 only
    assert call(np.float32, step_du=(0, 1e38)) == (S().SF_ERR_INVALID, -7)
    assert call(np.float64, step_du=(0, 1e38))[0] == S().SF_OK
    assert call(np.float32, view=dict(du=(1, 1e38))) == (S().SF_ERR_INVALID, -7)
    assert call(np.float32, view=dict(step=(2, 1e39))) == (S().SF_ERR_INVALID, -7)
    assert call(np.float64, view=dict(step=(2, 1e39))) == (S().SF_OK, CR.UP)


def test_driver_parses_render_camera_before_the_device():
    usage = "--render-camera takes EX,EY,EZ:TX,TY,TZ:WxH:SIGMA[:FOV_DEG[:STEP]]"
    for good in ("1,2,3:20,20,20:64x48:4", "0,0,-40:17,17,17:8x8:0", "-2,1,-1:9,9,9:1x1:2.5:60", "1e0,1.5,0:5,5,5:16384x1:4:40:1.7"):
        out = subprocess.run([EXE, "--render-camera", good, "--bogus"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (good, out.returncode, out.stderr)
    for bad in ("", "1,2,3", "1,2,3:4,5,6", "1,2,3:4,5,6:64x48", "1,2:4,5,6:64x48:4", "1,2,3:4,5:64x48:4", "1,2,3,4:4,5,6:64x48:4",
                "1,2,3:1,2,3:64x48:4", "1,2,nan:4,5,6:64x48:4", "1,2,3:4,5,inf:8x8:4", "1,2,3:4,5,6:64:4", "1,2,3:4,5,6:0x48:4",
                "1,2,3:4,5,6:64x0:4", "1,2,3:4,5,6:16385x4:4", "1,2,3:4,5,6:64x48:-1", "1,2,3:4,5,6:64x48:nan",
                "1,2,3:4,5,6:64x48:4x", "1,2,3:4,5,6:64x48:", "1,2,3:4,5,6:64x48:4:0", "1,2,3:4,5,6:64x48:4:180",
                "1,2,3:4,5,6:64x48:4:-20", "1,2,3:4,5,6:64x48:4:40:0", "1,2,3:4,5,6:64x48:4:40:-1", "1,2,3:4,5,6:64x48:4:40:",
                "1,2,3:4,5,6:64x48:4:40:1:2", "1,,3:4,5,6:64x48:4", "a,b,c:4,5,6:64x48:4"):
        out = subprocess.run([EXE, "--render-camera", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and usage in out.stderr, (bad, out.returncode, out.stderr)
    out = subprocess.run([EXE, "--render-camera"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "missing value" in out.stderr, (out.returncode, out.stderr)


def test_driver_lists_render_camera_in_its_usage():
    out = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--render-camera EX,EY,EZ:TX,TY,TZ:WxH:SIGMA[:FOV_DEG[:STEP]]" in out.stdout, (out.returncode, out.stdout)
