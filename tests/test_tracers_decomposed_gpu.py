"""Tracers on slab-decomposed contexts (docs/SPEC.md §6.1): ownership by the sampled plane, migration to the
neighbouring slab through the ghost-plane transports, and output in id order. Every comparison is exact equality of the
bits (gpu_support.assert_same_bits), against the CPU oracle and against the undecomposed context."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from gpu_support import DT, DTYPES, NAMES, ROOT, S, assert_same_bits, make

pytestmark = pytest.mark.gpu


def owner(z, N, nzl):
    """SPEC §6.1: the slab whose planes the sample reads (k0 as the trilinear sampler computes it)."""
    z = np.clip(np.nan_to_num(z, nan=0.0), 0.5, N + 0.5)
    k0 = np.clip(z.astype(np.int64), 0, N)
    return np.where(k0 == 0, 0, (k0 - 1) // nzl)


def tracer_inputs(N, P, dtype, n=2000, seed=7):
    """Random fields whose w moves a tracer by at most ~0.9 of a slab per call (N = 24, P <= 4: nzl >= 6), and tracers
    inside and outside the box, on slab boundary planes and on the 0.5 / N + 0.5 clamp planes."""
    rng = np.random.RandomState(seed)
    f = {n_: (0.2 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n_ in NAMES}
    nzl = N // P
    vmax = 0.9 * nzl / (DT * N)
    for c in ("u", "v", "w"):
        f[c] = np.clip(rng.standard_normal((N + 2,) * 3) * 0.5 * vmax, -vmax, vmax).astype(dtype)
    pos = rng.uniform(-1.0, N + 2.0, size=(n, 3))
    m = n // 8
    pos[:m, 2] = rng.randint(0, P + 1, size=m) * nzl + rng.choice([0.0, 1.0, 0.5], size=m)  # on slab boundary planes
    pos[m:2 * m, 2] = rng.choice([0.5, N + 0.5], size=m)
    pos[2 * m:3 * m, 0] = rng.choice([0.5, N + 0.5], size=m)
    return f, pos.astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("transport", ["copy", "rccl-self"])
@pytest.mark.parametrize("P", [2, 3, 4])
def test_tracers_parity_with_oracle_and_one_slab(P, transport, dtype):
    N, calls = 24, 5
    f, pos = tracer_inputs(N, P, dtype)
    nzl = N // P
    want = pos.copy()
    hist = [owner(want[:, 2].astype(np.float64), N, nzl)]
    for _ in range(calls):
        O.tracers_advect(want, f["u"], f["v"], f["w"], dtype(DT))
        hist.append(owner(want[:, 2].astype(np.float64), N, nzl))
    want_d, want_s = O.tracers_sample(want, f["dens"], f["u"], f["v"], f["w"])
    steps = np.diff(np.stack(hist), axis=0)
    assert (steps == 1).any() and (steps == -1).any(), "the inputs must move tracers up and down across slabs"
    assert np.abs(steps).max() <= 1

    out = {}
    for p in (1, P):
        with make(N, dtype, P=p, transport=transport) as fs:
            for k in ("u", "v", "w", "dens"):
                fs.upload(k, f[k])
            fs.tracers_set(pos)
            g0 = fs.transport_info()["rccl_groups"]
            for _ in range(calls):
                fs.tracers_advect()
            out[p] = fs.tracers_get()
            fs.sync()
            if p > 1 and transport == "rccl-self":
                assert fs.transport_info()["rccl_groups"] - g0 == calls
            assert fs.tracers_owned() == len(pos)
    for q, (what, w) in enumerate((("positions", want), ("density", want_d), ("speed", want_s))):
        assert_same_bits(out[P][q], w, f"P={P} {transport}: {what} vs oracle")
        assert_same_bits(out[P][q], out[1][q], f"P={P} {transport}: {what} vs one slab")


def test_set_then_get_returns_raw_positions():
    N, P = 24, 4
    _, pos = tracer_inputs(N, P, np.float32, n=500)
    pos[0] = (np.nan, -3.0, 1e9)
    with make(N, np.float32, P=P) as fs:
        fs.tracers_set(pos)
        got = fs.tracers_get(sample=False)[0]
    np.testing.assert_array_equal(got, pos)


@pytest.mark.parametrize("transport", ["copy", "rccl-self"])
def test_tracers_with_full_steps(transport):
    N, P, K, rounds = 32, 4, 4, 6
    rng = np.random.RandomState(3)
    f = {n: (0.2 * rng.standard_normal((N + 2,) * 3)).astype(np.float32) for n in NAMES}
    lim = 0.9 / (DT * N) / 4  # |dt N w| < 1: advect stays inside one ghost plane (SPEC §4)
    for c in ("u", "v", "w", "u0", "v0", "w0"):
        f[c] = np.clip(f[c], -lim, lim).astype(np.float32)
    pos = rng.uniform(0.0, N + 1.0, size=(3000, 3)).astype(np.float32)
    out = {}
    for p in (1, P):
        with make(N, np.float32, K=K, P=p, transport=transport) as fs:
            for n in NAMES:
                fs.upload(n, f[n])
            fs.tracers_set(pos)
            for _ in range(rounds):
                fs.vel_step()
                fs.dens_step()
                fs.tracers_advect()
            out[p] = fs.tracers_get()
            fs.sync()
    for q, what in enumerate(("positions", "density", "speed")):
        assert_same_bits(out[P][q], out[1][q], f"{transport}: {what} after {rounds} full steps")


def test_get_owned_on_four_slabs():
    N, P = 24, 4
    f, pos = tracer_inputs(N, P, np.float32, n=1500)
    with make(N, np.float32, P=P) as fs:
        for k in ("u", "v", "w", "dens"):
            fs.upload(k, f[k])
        fs.tracers_set(pos)
        fs.tracers_advect()
        fs.tracers_advect()
        xyz, dens, speed = fs.tracers_get()
        ids, oxyz, odens, ospeed = fs.tracers_get_owned()
        kb, ke = fs.owned_planes()
    assert (kb, ke) == (1, N + 1)
    np.testing.assert_array_equal(ids, np.arange(len(pos)))
    assert_same_bits(oxyz, xyz, "owned positions")
    assert_same_bits(odens, dens, "owned density")
    assert_same_bits(ospeed, speed, "owned speed")


def test_get_owned_per_slab_of_a_rank_share():
    """Loopback rank share (rank 1 of 4, no communicator): the context keeps what its slab owns, in id order. Its
    migrants come back to it as the loopback's arrivals, far outside its planes: their samples must stay inside the
    slab's buffers. sf_tracers_get refuses on several ranks."""
    N, nranks = 32, 4
    rng = np.random.RandomState(9)
    pos = rng.uniform(0.0, N + 1.0, size=(4096, 3)).astype(np.float32)
    Sx = S()
    with Sx.FluidSolver(N, dtype="f32", iters=4, rank=1, nranks=nranks, flags=Sx.SF_FLAG_LOOPBACK_HALO) as fs:
        kb, ke = fs.owned_planes()
        skb, ske = fs.stored_planes()
        z = np.zeros((ske - skb, N + 2, N + 2), np.float32)
        for n in NAMES:
            fs.upload_planes(n, skb, z + {"dens": 0.25, "w": 1.0}.get(n, 0.0))  # dt N w = 3.2 planes up per call
        fs.tracers_set(pos)
        ids, xyz, dens, _ = fs.tracers_get_owned()
        k0 = np.clip(np.clip(xyz[:, 2], 0.5, N + 0.5).astype(np.int64), 0, N)
        assert len(ids) > 0 and np.all(np.diff(ids) > 0)
        assert np.all((k0 >= kb) & (k0 < ke))
        want_ids = np.nonzero(owner(pos[:, 2].astype(np.float64), N, N // nranks) == 1)[0]
        np.testing.assert_array_equal(ids, want_ids)
        np.testing.assert_array_equal(xyz, pos[ids])
        assert np.isfinite(dens).all()
        for _ in range(2):
            fs.tracers_advect()
        fs.sync()
        ids2, xyz2, dens2, _ = fs.tracers_get_owned()
        assert len(ids2) <= len(pos) and np.all(np.diff(ids2) > 0)
        assert len(ids2) == len(ids)  # the loopback hands every migrant back
        assert np.isfinite(xyz2).all() and np.isfinite(dens2).all()
        assert (xyz2[:, 2] > ke).any()  # some did leave the slab
        with pytest.raises(Sx.SfError) as e:
            fs.tracers_get()
        assert e.value.status == Sx.SF_ERR_INVALID and "sf_tracers_get_owned" in str(e.value)


def test_capacity_overflow_is_reported_and_recoverable():
    N, P = 24, 4
    f, pos = tracer_inputs(N, P, np.float32, n=2000)
    f["w"][...] = 2.0  # dt N w = 4.8 planes up per call: many tracers cross, none skips a slab of 6
    Sx = S()
    with make(N, np.float32, P=P) as fs:
        for k in ("u", "v", "w", "dens"):
            fs.upload(k, f[k])
        fs.tracers_set(pos)
        fs.tracers_set_capacity(1)
        fs.tracers_advect()
        with pytest.raises(Sx.SfError) as e:
            fs.sync()
        assert e.value.status == Sx.SF_ERR_TRACER_OVERFLOW
        fs.sync()  # reported once
        assert fs.tracers_owned() == len(pos)  # nothing dropped
        fs.tracers_set_capacity(len(pos))
        fs.tracers_set(pos)
        fs.tracers_advect()
        got = fs.tracers_get()
        fs.sync()
    want = pos.copy()
    O.tracers_advect(want, f["u"], f["v"], f["w"], np.float32(DT))
    want_d, want_s = O.tracers_sample(want, f["dens"], f["u"], f["v"], f["w"])
    assert_same_bits(got[0], want, "positions after re-set")
    assert_same_bits(got[1], want_d, "density after re-set")
    assert_same_bits(got[2], want_s, "speed after re-set")


def test_tracer_skipping_a_slab_is_reported():
    N, P = 8, 8  # one plane per slab
    f, pos = tracer_inputs(N, P, np.float32, n=200)
    f["w"][...] = 3.0  # dt N w = 2.4 planes
    Sx = S()
    with make(N, np.float32, P=P) as fs:
        for k in ("u", "v", "w", "dens"):
            fs.upload(k, f[k])
        fs.tracers_set(pos)
        fs.tracers_advect()
        with pytest.raises(Sx.SfError) as e:
            fs.sync()
        assert e.value.status == Sx.SF_ERR_HALO_EXCEEDED and "tracer" in str(e.value)
        fs.sync()
        assert fs.tracers_owned() == len(pos)


def _driver(args, out_dir):
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    cmd = [exe, "--iters", "6", "--quiet", "--out", str(out_dir)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_driver_slab_tracer_frames_equal_the_single_slab_frames(tmp_path):
    base = ["--n", "48", "--steps", "3", "--every", "2", "--binary", "--tracers", "1000"]
    frames = {}
    for tag, extra in (("one", []), ("four", ["--slabs", "4"]), ("four-sync", ["--slabs", "4", "--sync-output"])):
        _driver(base + extra, tmp_path / tag)
        frames[tag] = [open(tmp_path / tag / f"tracers_s{q}.vtk", "rb").read() for q in (0, 1)]
    assert len(frames["one"][0]) > 1000
    assert frames["four"] == frames["one"] and frames["four-sync"] == frames["one"]


def test_driver_rank_share_writes_its_tracer_file(tmp_path):
    _driver(["--steps", "1", "--every", "1", "--loopback", "--rank", "1", "--world", "4", "--tracers", "4096"], tmp_path)
    data = open(tmp_path / "tracers_s_GPU1_0.vtk").read()
    assert "POINTS" in data and "density" in data
