"""CPU side of orthographic volume rendering (docs/SPEC.md §13): the three entry points are declared, exported and
wrapped, sf_view_params agrees between include/sfgpu.h and the ctypes mirror, sf_view_frame rejects what it must and
equals the numpy camera in bits, and the driver takes --render-view before it touches the device. No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np

import render_view_ref as VR
from abi_header import ROOT, declared_functions, header_text, struct_members

SYMBOLS = ("sf_render_view", "sf_render_view_read", "sf_view_frame")
EXE = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")


def S():
    from fluidsolvergpu_amd import solver

    return solver


def c_frame(N, d, up, W, H, step, sigma):
    f = S().SfViewParams()
    rc = S().lib.sf_view_frame(N, (C.c_double * 3)(*d), (C.c_double * 3)(*up), W, H, step, sigma, C.byref(f))
    return rc, f


def test_symbols_declared_exported_and_wrapped():
    for name in SYMBOLS:
        assert name in declared_functions("sfgpu.h"), f"sfgpu.h does not declare {name}"
        assert name in S().ABI_SYMBOLS
        assert hasattr(S().lib, name), f"libsfgpu.so does not export {name}"
    for method in ("view_frame", "render_view"):
        assert callable(getattr(S().FluidSolver, method))


def test_struct_layout_matches_the_header():
    members = struct_members(header_text(), "sf_view_params")
    assert members == [("origin[3]", "double"), ("du[3]", "double"), ("dv[3]", "double"), ("step[3]", "double"),
                       ("width", "int"), ("height", "int"), ("samples", "int"), ("sigma", "double"), ("dens", "int"),
                       ("emit", "int")]
    want = {"int": C.c_int, "double": C.c_double}
    mirror = [(n, t) for n, t in S().SfViewParams._fields_]
    assert [n for n, _ in mirror] == [n.split("[")[0] for n, _ in members]
    for (n, t), (hn, ht) in zip(mirror, members):
        assert t is (want[ht] * 3 if hn.endswith("[3]") else want[ht]), n
    assert C.sizeof(S().SfViewParams) == 128
    assert [getattr(S().SfViewParams, n).offset for n, _ in mirror] == [0, 24, 48, 72, 96, 100, 104, 112, 120, 124]


def test_entry_points_reject_null_pointers():
    p = S().SfViewParams()
    assert S().lib.sf_render_view(None, C.byref(p)) == S().SF_ERR_INVALID
    assert S().lib.sf_render_view(None, None) == S().SF_ERR_INVALID
    assert S().lib.sf_render_view_read(None, None, None) == S().SF_ERR_INVALID
    d, up = (C.c_double * 3)(1, 2, 3), (C.c_double * 3)(0, 0, 1)
    L = S().lib
    assert L.sf_view_frame(8, None, up, 4, 4, 1.0, 1.0, C.byref(p)) == S().SF_ERR_INVALID
    assert L.sf_view_frame(8, d, None, 4, 4, 1.0, 1.0, C.byref(p)) == S().SF_ERR_INVALID
    assert L.sf_view_frame(8, d, up, 4, 4, 1.0, 1.0, None) == S().SF_ERR_INVALID
    assert L.sf_view_frame(8, d, up, 4, 4, 1.0, 1.0, C.byref(p)) == S().SF_OK


def test_view_frame_rejects_what_it_must():
    nan, inf = float("nan"), float("inf")
    good = dict(N=8, d=(1, 2, 3), up=(0, 0, 1), W=4, H=5, step=1.0, sigma=1.0)
    assert c_frame(**good)[0] == S().SF_OK
    assert c_frame(**{**good, "sigma": 0.0})[0] == S().SF_OK
    assert c_frame(**{**good, "W": 16384, "H": 1})[0] == S().SF_OK
    for bad in (dict(d=(0, 0, 0)), dict(d=(0, 0, 2), up=(0, 0, 1)), dict(d=(1, 2, 3), up=(-2, -4, -6)), dict(up=(0, 0, 0)),
                dict(d=(nan, 0, 1)), dict(d=(inf, 0, 1)), dict(up=(0, nan, 1)), dict(step=0.0), dict(step=-1.0),
                dict(step=nan), dict(step=inf), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(W=0), dict(H=0),
                dict(W=16385), dict(H=16385), dict(W=-3), dict(step=1e-4), dict(N=0)):
        rc, f = c_frame(**{**good, **bad})
        assert rc == S().SF_ERR_INVALID, bad


def test_view_frame_equals_the_numpy_camera_in_bits():
    rng = np.random.RandomState(1300)
    dirs = [(1, 2, 3), (-2, 1, -1), (1, 1, 0), (3, -1, 2), (0, 0, 1), (0, 0, -1), (1, 0, 0), (0, -1, 0)]
    dirs += [tuple(rng.standard_normal(3)) for _ in range(12)]
    assert len(dirs) == 20
    for n, d in enumerate(dirs):
        up = (0, 1, 0) if d[0] == 0 and d[1] == 0 else (0, 0, 1)
        N, W, H = (1, 5, 34, 130, 1024)[n % 5], (1, 7, 64, 513)[n % 4], (1, 9, 65)[n % 3]
        step, sigma = (0.5, 1.0, 1.7)[n % 3], (0.0, 4.0, 0.3)[(n // 3) % 3]
        rc, f = c_frame(N, d, up, W, H, step, sigma)
        assert rc == S().SF_OK
        fr = VR.view_frame(N, d, up, W, H, step, sigma)
        for name, want in (("origin", fr.origin), ("du", fr.du), ("dv", fr.dv), ("step", fr.step)):
            got = np.array(getattr(f, name)[:], np.float64)
            assert got.tobytes() == np.asarray(want, np.float64).tobytes(), (d, name, got, want)
        assert np.float64(f.sigma).tobytes() == np.float64(fr.sigma).tobytes()
        assert (f.width, f.height, f.samples, f.dens, f.emit) == (W, H, fr.samples, -1, -1)


def test_driver_parses_render_view_before_the_device():
    for good in ("1,2,3:64x48:4", "0,0,1:8x8:0", "-2,1,-1:1x1:2.5:0.5", "1e0,1.5,0:16384x1:4:1.7"):
        out = subprocess.run([EXE, "--render-view", good, "--bogus"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "unknown option --bogus" in out.stderr, (good, out.returncode, out.stderr)
    for bad in ("", "1,2,3", "1,2,3:64x48", "1,2:64x48:4", "1,2,3,4:64x48:4", "0,0,0:64x48:4", "1,2,nan:64x48:4",
                "1,2,inf:8x8:4", "1,2,3:64:4", "1,2,3:0x48:4", "1,2,3:64x0:4", "1,2,3:16385x4:4", "1,2,3:64x48x2:4",
                "1,2,3:64x48:-1", "1,2,3:64x48:nan", "1,2,3:64x48:4x", "1,2,3:64x48:", "1,2,3:64x48:4:0", "1,2,3:64x48:4:-1",
                "1,2,3:64x48:4:", "1,2,3:64x48:4:1:2", "1,,3:64x48:4", "a,b,c:64x48:4", "1,2,3:-4x48:4"):
        out = subprocess.run([EXE, "--render-view", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--render-view takes DX,DY,DZ:WxH:SIGMA[:STEP]" in out.stderr, (bad, out.returncode,
                                                                                                   out.stderr)
    out = subprocess.run([EXE, "--render-view"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "missing value" in out.stderr, (out.returncode, out.stderr)


def test_driver_lists_render_view_in_its_usage():
    out = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--render-view DX,DY,DZ:WxH:SIGMA[:STEP]" in out.stdout, (out.returncode, out.stdout)
    out = subprocess.run([EXE, "--bogus"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--render-view DX,DY,DZ:WxH:SIGMA[:STEP]" in out.stderr
