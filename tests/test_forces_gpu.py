"""External forces on the GPU (docs/SPEC.md §8): vorticity confinement and buoyancy through libsfgpu.so, against the
numpy reference (tests/forces_ref.py) followed by the CPU oracle. Every comparison is exact bit equality over all 8
fields (and the user slots involved), shells included."""
import os
import subprocess

import numpy as np
import pytest

import forces_ref as F
import oracle_lib as O
from gpu_support import (DIFF, DT, DTYPES, NAMES, OPERATOR_CASES, OPERATOR_IDS, ROOT, USER, VISC, S, assert_same_bits,
                         bench_state, check_all, make, random_fields, set_forces, upload_all)

pytestmark = pytest.mark.gpu


# ---- the two passes singly -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,P,transport", OPERATOR_CASES, ids=OPERATOR_IDS)
def test_operators_match_reference(N, P, transport, dtype):
    f = random_fields(N, dtype, 11 + N + P, vel=1.0)
    eps, beta, amb, axis = 0.35, 1.7, 0.1, 2
    want = {n: a.copy() for n, a in f.items()}
    want["user0"] = F.vorticity(f["u"], f["v"], f["w"])
    F.add_forces(want["u"], want["v"], want["w"], want["dens"], want["u0"], want["v0"], want["w0"], eps, beta, amb,
                 axis)
    with make(N, dtype, P=P, transport=transport) as fs:
        upload_all(fs, f)
        fs.upload("user0", np.full((N + 2,) * 3, 7.0, dtype))
        fs.vorticity_magnitude("u", "v", "w", "user0")
        fs.set_vorticity_confinement(eps)
        fs.set_buoyancy(beta, amb, axis)
        fs.add_forces("u", "v", "w", "dens", "u0", "v0", "w0")
        check_all(fs, want, f"N={N} P={P} {transport}", NAMES + ("user0",))
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


# ---- full steps --------------------------------------------------------------------------------------------------
FORCES = {"vort": dict(eps=0.3), "buoy": dict(beta=2.0, ambient=0.05, axis=1), "both": dict(eps=0.3, beta=-1.5,
                                                                                               ambient=0.0, axis=2)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("bound", [False, True], ids=["unbound", "bound"])
@pytest.mark.parametrize("mode", list(FORCES))
def test_steps_match_reference(mode, bound, P, dtype):
    N, K, steps = 24, 4, 3
    f = random_fields(N, dtype, 3 + P)
    rng = np.random.RandomState(9)
    src = {n: (0.2 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in USER}
    want = {n: a.copy() for n, a in f.items()}
    with make(N, dtype, K=K, P=P) as fs:
        upload_all(fs, f)
        if bound:
            for n, slot in USER.items():
                fs.upload(slot, src[n])
            fs.bind_sources()
        set_forces(fs, **FORCES[mode])
        for s in range(steps):
            fs.vel_step()
            fs.dens_step()
            F.step(want, DT, DIFF, VISC, K, bound=src if bound else None, **FORCES[mode])
            check_all(fs, want, f"{mode} {'bound' if bound else 'unbound'} P={P} step {s}")
        if bound:
            for n, slot in USER.items():
                assert_same_bits(fs.download(slot), src[n], f"bound slot {slot} after the steps")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_forces_off_again_is_the_plain_step(dtype):
    N, K = 24, 4
    f = random_fields(N, dtype, 21)
    want = {n: a.copy() for n, a in f.items()}
    for _ in range(2):
        O.step(N, want, dtype(DT), dtype(DIFF), dtype(VISC), K)
    with make(N, dtype, K=K, P=2) as a, make(N, dtype, K=K, P=2) as b:
        for fs in (a, b):
            upload_all(fs, f)
        set_forces(a, eps=0.5, beta=3.0, ambient=1.0, axis=0)
        set_forces(a, eps=0.0, beta=0.0, ambient=1.0, axis=0)
        for fs in (a, b):
            for _ in range(2):
                fs.vel_step()
                fs.dens_step()
        check_all(a, want, "forces switched off")
        check_all(b, want, "forces never set")


def test_marching_path_256_with_forces():
    """256^3 fp32 K = 20 (the size classes above ~136^3 run the marching Jacobi kernel), SPEC §5 inputs with bound
    sources plus both forces: one step against the oracle."""
    N, K, dtype = 256, 20, np.float32
    forces = dict(eps=0.25, beta=0.8, ambient=0.5, axis=1)
    f, src = bench_state(N, dtype)
    with make(N, dtype, K=K) as fs:
        for n in ("u", "v", "w", "dens"):
            fs.upload(n, f[n])
        for n, slot in USER.items():
            fs.upload(slot, src[n])
        fs.bind_sources()
        set_forces(fs, **forces)
        fs.vel_step()
        fs.dens_step()
        fs.sync()
        want = {n: f[n] for n in ("u", "v", "w", "dens")}
        z = np.zeros((N + 2,) * 3, dtype)
        want.update({n: z.copy() for n in USER})
        F.step(want, DT, DIFF, VISC, K, bound=src, **forces)
        check_all(fs, want, "256^3 K=20 with forces")


def test_graph_replay_tracks_the_force_coefficients(monkeypatch):
    monkeypatch.setenv("SF_GRAPH", "1")
    N, K, dtype = 32, 4, np.float32
    f = random_fields(N, dtype, 31)
    rng = np.random.RandomState(32)
    src = {n: (0.2 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in USER}
    want = {n: a.copy() for n, a in f.items()}
    with make(N, dtype, K=K) as fs:
        upload_all(fs, f)
        for n, slot in USER.items():
            fs.upload(slot, src[n])
        fs.bind_sources()
        for s, eps in enumerate((0.3, 0.3, 0.6, 0.3, 0.6, 0.0)):
            set_forces(fs, eps=eps, beta=1.0, ambient=0.0, axis=1)
            fs.vel_step()
            fs.dens_step()
            F.step(want, DT, DIFF, VISC, K, bound=src, eps=eps, beta=1.0, ambient=0.0, axis=1)
            check_all(fs, want, f"SF_GRAPH=1 step {s} eps={eps}")


# ---- closed forms of SPEC §8 through the C ABI ---------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_closed_forms_through_the_abi(dtype, P):
    N, eps = 32, 0.3
    k, j, i = np.meshgrid(*(np.arange(N + 2, dtype=np.float64),) * 3, indexing="ij")
    zero = np.zeros((N + 2,) * 3, dtype)
    c = N // 2
    profiles = {"shear": (zero, (i * i).astype(dtype), zero), "rotation": ((c - j).astype(dtype), (i - c).astype(dtype),
                                                                          zero)}
    with make(N, dtype, P=P) as fs:
        fs.set_vorticity_confinement(eps)
        for name, (u, v, w) in profiles.items():
            for n, a in (("u", u), ("v", v), ("w", w), ("dens", zero), ("u0", zero), ("v0", zero), ("w0", zero)):
                fs.upload(n, a)
            fs.vorticity_magnitude("u", "v", "w", "user0")
            fs.add_forces("u", "v", "w", "dens", "u0", "v0", "w0")
            fs.sync()
            mag = fs.download("user0")
            assert_same_bits(mag, F.vorticity(u, v, w), f"{name}: |omega|")
            su, sv, sw = zero.copy(), zero.copy(), zero.copy()
            F.add_forces(u, v, w, zero, su, sv, sw, eps=eps)
            for n, ref in (("u0", su), ("v0", sv), ("w0", sw)):
                assert_same_bits(fs.download(n), ref, f"{name}: {n}")
            if name == "shear":
                assert np.array_equal(mag[1:-1, 1:-1, 1:-1], np.broadcast_to(2 * N * np.arange(1, N + 1), (N, N, N)))
                assert not fs.download("u0").any() and not fs.download("w0").any()
                fy = fs.download("v0")[1:-1, 1:-1, 1:-1].astype(np.float64)
                want = -2.0 * eps * np.arange(1, N + 1)
                assert np.all(np.abs(fy - want) <= 8 * np.finfo(dtype).eps * np.abs(want))
            else:
                assert (mag[1:-1, 1:-1, 1:-1] == 2 * N).all()
                assert not fs.download("u0").any() and not fs.download("v0").any() and not fs.download("w0").any()


def test_invalid_arguments_leave_the_context_working():
    N, K, dtype = 16, 4, np.float32
    solver = S()
    f = random_fields(N, dtype, 41)
    want = {n: a.copy() for n, a in f.items()}
    F.step(want, DT, DIFF, VISC, K, eps=0.2)
    with make(N, dtype, K=K) as fs:
        upload_all(fs, f)
        fs.set_vorticity_confinement(0.2)
        bad = [lambda: fs.set_vorticity_confinement(-0.1), lambda: fs.set_vorticity_confinement(float("nan")),
               lambda: fs.set_vorticity_confinement(float("inf")), lambda: fs.set_buoyancy(1.0, 0.0, 3),
               lambda: fs.set_buoyancy(1.0, 0.0, -1), lambda: fs.set_buoyancy(float("nan"), 0.0, 1),
               lambda: fs.set_buoyancy(1.0, float("inf"), 1), lambda: fs.vorticity_magnitude("u", "v", "w", "v"),
               lambda: fs.vorticity_magnitude("u", "v", "w", 12), lambda: fs.vorticity_magnitude(-1, "v", "w", "user0"),
               lambda: fs.add_forces("u", "v", "w", "dens", "u0", "v0", "u"),
               lambda: fs.add_forces("u", "v", "w", "dens", "u0", "u0", "w0"),
               lambda: fs.add_forces("u", "v", "w", "dens", "u0", "v0", 12)]
        for call in bad:
            with pytest.raises(solver.SfError) as e:
                call()
            assert e.value.status == solver.SF_ERR_INVALID
        fs.vel_step()
        fs.dens_step()
        check_all(fs, want, "after rejected calls")


def test_driver_frames_with_forces(tmp_path):
    """sf_driver --vorticity / --buoyancy (bound sources, SPEC §5 plumbing inputs): the frames are the bytes of the
    reference fields written by fluidsolvergpu_amd.vtk."""
    from fluidsolvergpu_amd import vtk as sfvtk

    N, K, steps = 32, 20, 2
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    cmd = [exe, "--plumbing", "--n", str(N), "--steps", str(steps), "--every", "1", "--binary", "--vorticity", "0.3",
           "--buoyancy", "2", "--quiet", "--out", str(tmp_path / "drv")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    z = lambda: np.zeros((N + 2,) * 3, np.float32)
    f = {n: z() for n in NAMES}
    src = {n: z() for n in USER}
    c = N // 2
    src["v0"][c, c, c] = 5.0
    src["dens0"][c, c, c] = 100.0
    for s in range(steps):
        F.step(f, DT, DIFF, VISC, K, bound=src, eps=0.3, beta=2.0, ambient=0.0, axis=1)
        dens = np.ascontiguousarray(f["dens"][1:-1, 1:-1, 1:-1]).ravel()
        vel = np.stack([f[n][1:-1, 1:-1, 1:-1] for n in ("u", "v", "w")], -1).ravel()
        p = str(tmp_path / f"ref_{s}.vtk")
        sfvtk.write_regular_mesh(p, 1, [N + 1] * 3, 2, [1, 3], [0, 0], ["density", "velocity"], [dens, vel])
        got = open(tmp_path / "drv" / f"anim_s{s}.vtk", "rb").read()
        assert got == open(p, "rb").read(), f"frame {s} differs"
