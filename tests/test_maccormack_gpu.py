"""MacCormack advection on the GPU (docs/SPEC.md §9): sf_advect_maccormack and the steps with sf_set_advection through
libsfgpu.so, against the numpy reference (tests/maccormack_ref.py, built on the CPU oracle). Every comparison is exact
bit equality over all fields, shells included."""
import os
import subprocess

import numpy as np
import pytest

import maccormack_ref as M
import oracle_lib as O
from gpu_support import (DIFF, DT, DTYPES, NAMES, OPERATOR_CASES, OPERATOR_IDS, ROOT, USER, VISC, S, assert_same_bits,
                         bench_state, check_all, make, random_fields, upload_all)

pytestmark = pytest.mark.gpu

SL, MC = M.SEMI_LAGRANGIAN, M.MACCORMACK
SCHEMES = {"vel": (MC, SL), "dens": (SL, MC), "both": (MC, MC)}


# ---- the operator singly -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,P,transport", OPERATOR_CASES, ids=OPERATOR_IDS)
def test_operator_matches_reference(N, P, transport, dtype):
    """b = 0..3 on random fields; u and v trace over several cells, |dt*N*w| < 1 (one ghost plane)."""
    rng = np.random.RandomState(100 + N + P)
    d0 = rng.standard_normal((N + 2,) * 3).astype(dtype)
    u, v = ((1.2 / (DT * N) * rng.standard_normal((N + 2,) * 3)).astype(dtype) for _ in range(2))
    w = (0.95 / (DT * N) * rng.uniform(-1, 1, (N + 2,) * 3)).astype(dtype)
    assert float(np.abs(dtype(DT) * dtype(N) * w).max()) < 1
    with make(N, dtype, P=P, transport=transport) as fs:
        for n, a in (("dens0", d0), ("u", u), ("v", v), ("w", w)):
            fs.upload(n, a)
        for b in range(4):
            fs.upload("dens", np.full((N + 2,) * 3, 7.0, dtype))
            fs.advect_maccormack(b, "dens", "dens0", "u", "v", "w")
            fs.sync()
            want = M.advect_mc(b, np.zeros_like(d0), d0, u, v, w, DT)
            assert_same_bits(fs.download("dens"), want, f"N={N} P={P} {transport} b={b}")
        for n, a in (("dens0", d0), ("u", u), ("v", v), ("w", w)):
            assert_same_bits(fs.download(n), a, f"input {n} after the operator")
        if transport == "rccl-self":
            assert fs.transport_info()["rccl_groups"] > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,sigma", [(40, 0.3), (64, 0.5)])
def test_operator_takes_every_branch(N, sigma, dtype):
    """Traces of several cells at P = 1: the comparison covers the wall fallback, the limiter and the unlimited value,
    each on a share of the interior that the reference confirms first."""
    rng = np.random.RandomState(5)
    d0 = rng.standard_normal((N + 2,) * 3).astype(dtype)
    u, v, w = ((sigma * rng.standard_normal((N + 2,) * 3)).astype(dtype) for _ in range(3))
    fallback, limited, unlimited = M.outcomes(d0, u, v, w, DT)
    print(f"N={N} sigma={sigma} {np.dtype(dtype).name}: fallback {fallback:.3f} limited {limited:.3f} "
          f"unlimited {unlimited:.3f}")
    assert fallback >= 0.05 and unlimited >= 0.05 and limited >= 0.02
    with make(N, dtype) as fs:
        for n, a in (("user0", d0), ("u0", u), ("v0", v), ("w0", w)):
            fs.upload(n, a)
        for b in range(4):
            fs.advect_maccormack(b, "user1", "user0", "u0", "v0", "w0")
            fs.sync()
            assert_same_bits(fs.download("user1"), M.advect_mc(b, np.zeros_like(d0), d0, u, v, w, DT), f"b={b}")


# ---- full steps --------------------------------------------------------------------------------------------------
# every scheme on 1..5 slabs, bound and unbound sources alternating so that each scheme sees both
STEP_CASES = [(mode, P, (P + q) % 2 == 1) for q, mode in enumerate(SCHEMES) for P in (1, 2, 3, 4, 5)]


def run_steps(fs, want, K, steps, what, src=None, schemes=(SL, SL), forces=None):
    fs.set_advection(*schemes)
    for s in range(steps):
        fs.vel_step()
        fs.dens_step()
        M.step(want, DT, DIFF, VISC, K, velocity=schemes[0], density=schemes[1], bound=src, **(forces or {}))
        check_all(fs, want, f"{what} step {s}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode,P,bound", STEP_CASES,
                         ids=[f"{m}-P{p}-{'bound' if b else 'unbound'}" for m, p, b in STEP_CASES])
def test_steps_match_reference(mode, P, bound, dtype):
    N, K, steps = (20 if P == 5 else 24), 4, 3
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
        run_steps(fs, want, K, steps, f"{mode} P={P}", src if bound else None, SCHEMES[mode])
        if bound:
            for n, slot in USER.items():
                assert_same_bits(fs.download(slot), src[n], f"bound slot {slot} after the steps")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("P,transport", [(1, "copy"), (3, "copy"), (4, "rccl-self")])
def test_steps_with_forces_match_reference(P, transport, dtype):
    """Both schemes on together with vorticity confinement and buoyancy (SPEC §8), bound sources."""
    N, K = 24, 4
    forces = dict(eps=0.3, beta=-1.5, ambient=0.0, axis=2)
    f = random_fields(N, dtype, 13 + P)
    rng = np.random.RandomState(14)
    src = {n: (0.2 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in USER}
    want = {n: a.copy() for n, a in f.items()}
    with make(N, dtype, K=K, P=P, transport=transport) as fs:
        upload_all(fs, f)
        for n, slot in USER.items():
            fs.upload(slot, src[n])
        fs.bind_sources()
        fs.set_vorticity_confinement(forces["eps"])
        fs.set_buoyancy(forces["beta"], forces["ambient"], forces["axis"])
        run_steps(fs, want, K, 3, f"forces P={P}", src, (MC, MC), forces)


_REF_256 = {}


def reference_256(dtype):
    """One step of the SPEC §5 inputs at 256^3, K = 20, both schemes on (computed once per precision)."""
    key = np.dtype(dtype).name
    if key not in _REF_256:
        N = 256
        f, src = bench_state(N, dtype)
        want = {n: f[n].copy() for n in ("u", "v", "w", "dens")}
        z = np.zeros((N + 2,) * 3, dtype)
        want.update({n: z.copy() for n in USER})
        M.step(want, DT, DIFF, VISC, 20, velocity=MC, density=MC, bound=src)
        _REF_256[key] = (f, src, want)
    return _REF_256[key]


@pytest.mark.parametrize("dtype,P", [(np.float32, 1), (np.float32, 4), (np.float64, 1), (np.float64, 4)],
                         ids=["f32-P1", "f32-P4", "f64-P1", "f64-P4"])
def test_full_size_256_step(dtype, P):
    N, K = 256, 20
    f, src, want = reference_256(dtype)
    with make(N, dtype, K=K, P=P) as fs:
        for n in ("u", "v", "w", "dens"):
            fs.upload(n, f[n])
        for n, slot in USER.items():
            fs.upload(slot, src[n])
        fs.bind_sources()
        fs.set_advection(MC, MC)
        fs.vel_step()
        fs.dens_step()
        check_all(fs, want, f"256^3 K=20 P={P}")


# ---- hipGraph replay ---------------------------------------------------------------------------------------------
def test_graph_replay_tracks_the_schemes(monkeypatch):
    """SF_GRAPH=1: a change of scheme between steps must capture anew, not replay the other scheme's launches. The
    graphed context is compared with one created without the switch, and both with the reference."""
    N, K, dtype = 32, 4, np.float32
    f = random_fields(N, dtype, 31)
    want = {n: a.copy() for n, a in f.items()}
    monkeypatch.setenv("SF_GRAPH", "1")
    graphed = make(N, dtype, K=K)
    monkeypatch.delenv("SF_GRAPH")
    plain = make(N, dtype, K=K)
    with graphed, plain:
        for fs in (graphed, plain):
            upload_all(fs, f)
        for s, schemes in enumerate([(SL, SL), (MC, SL), (MC, SL), (MC, MC), (SL, MC), (SL, SL), (MC, MC), (SL, MC)]):
            for fs in (graphed, plain):
                fs.set_advection(*schemes)
                fs.vel_step()
                fs.dens_step()
                fs.sync()
            M.step(want, DT, DIFF, VISC, K, velocity=schemes[0], density=schemes[1])
            for n in NAMES:
                assert_same_bits(graphed.download(n), plain.download(n), f"SF_GRAPH=1 step {s} {schemes}: {n} vs plain")
            check_all(graphed, want, f"SF_GRAPH=1 step {s} {schemes}")


# ---- errors and the default --------------------------------------------------------------------------------------
def test_reverse_trace_past_the_ghost_plane_is_reported():
    """P = 2: a large positive w in the lower slab. Its forward traces end at the k = 0 wall, inside the slab; its
    reverse traces run 4.8 planes upwards, past the ghost plane. Reported by sf_sync, never clamped silently."""
    N, dtype = 16, np.float32
    solver = S()
    f = random_fields(N, dtype, 11)
    f["w"][...] = 0
    f["w"][1:N // 2 + 1] = 3.0  # dt*N*w = 4.8 planes
    with make(N, dtype, P=2) as fs:
        upload_all(fs, f)
        fs.advect(0, "dens", "dens0", "u", "v", "w")
        fs.sync()  # the forward trace alone stays inside
        fs.advect_maccormack(0, "dens", "dens0", "u", "v", "w")
        with pytest.raises(solver.SfError) as e:
            fs.sync()
        assert e.value.status == solver.SF_ERR_HALO_EXCEEDED
        fs.sync()  # the flag is cleared once reported


def test_invalid_arguments_leave_the_context_working():
    N, K, dtype = 16, 4, np.float32
    solver = S()
    f = random_fields(N, dtype, 41)
    want = {n: a.copy() for n, a in f.items()}
    M.step(want, DT, DIFF, VISC, K, velocity=MC)
    with make(N, dtype, K=K) as fs:
        upload_all(fs, f)
        fs.set_advection(MC, SL)
        bad = [lambda: fs.set_advection(2, 0), lambda: fs.set_advection(0, -1), lambda: fs.set_advection(1, 7),
               lambda: fs.advect_maccormack(0, "dens", "dens", "u", "v", "w"),
               lambda: fs.advect_maccormack(1, "u", "u0", "u", "v", "w"),
               lambda: fs.advect_maccormack(0, "dens", "dens0", "u", "dens", "w"),
               lambda: fs.advect_maccormack(4, "dens", "dens0", "u", "v", "w"),
               lambda: fs.advect_maccormack(0, 12, "dens0", "u", "v", "w")]
        for call in bad:
            with pytest.raises(solver.SfError) as e:
                call()
            assert e.value.status == solver.SF_ERR_INVALID
        fs.vel_step()  # the schemes in force are still (MacCormack, first order)
        fs.dens_step()
        check_all(fs, want, "after rejected calls")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_default_and_switched_off_are_the_plain_step(dtype):
    N, K = 24, 4
    f = random_fields(N, dtype, 21)
    want = {n: a.copy() for n, a in f.items()}
    for _ in range(2):
        O.step(N, want, dtype(DT), dtype(DIFF), dtype(VISC), K)
    with make(N, dtype, K=K, P=2) as a, make(N, dtype, K=K, P=2) as b:
        for fs in (a, b):
            upload_all(fs, f)
        a.set_advection(MC, MC)
        a.set_advection(SL, SL)
        for fs in (a, b):
            for _ in range(2):
                fs.vel_step()
                fs.dens_step()
        check_all(a, want, "schemes switched off again")
        check_all(b, want, "schemes never set")


# ---- driver ------------------------------------------------------------------------------------------------------
def test_driver_frames_with_maccormack(tmp_path):
    """sf_driver --maccormack both (bound sources, SPEC §5 plumbing inputs): the frames of one slab are the bytes of
    the reference fields written by fluidsolvergpu_amd.vtk, and the frames of three slabs are the same bytes."""
    from fluidsolvergpu_amd import vtk as sfvtk

    N, K, steps = 24, 20, 2
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    for slabs in (1, 3):
        cmd = [exe, "--plumbing", "--n", str(N), "--steps", str(steps), "--every", "1", "--binary", "--maccormack",
               "both", "--slabs", str(slabs), "--quiet", "--out", str(tmp_path / f"drv{slabs}")]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
    z = lambda: np.zeros((N + 2,) * 3, np.float32)
    f = {n: z() for n in NAMES}
    src = {n: z() for n in USER}
    c = N // 2
    src["v0"][c, c, c] = 5.0
    src["dens0"][c, c, c] = 100.0
    for s in range(steps):
        M.step(f, DT, DIFF, VISC, K, velocity=MC, density=MC, bound=src)
        dens = np.ascontiguousarray(f["dens"][1:-1, 1:-1, 1:-1]).ravel()
        vel = np.stack([f[n][1:-1, 1:-1, 1:-1] for n in ("u", "v", "w")], -1).ravel()
        p = str(tmp_path / f"ref_{s}.vtk")
        sfvtk.write_regular_mesh(p, 1, [N + 1] * 3, 2, [1, 3], [0, 0], ["density", "velocity"], [dens, vel])
        one = open(tmp_path / "drv1" / f"anim_s{s}.vtk", "rb").read()
        three = open(tmp_path / "drv3" / f"anim_s{s}.vtk", "rb").read()
        assert one == open(p, "rb").read(), f"frame {s} differs from the reference"
        assert three == one, f"frame {s}: three slabs differ from one"
