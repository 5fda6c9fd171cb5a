"""GPU parity: libsfgpu.so (gfx950 HIP, through the C ABI) vs the CPU oracle, bit for bit.

The reference has no implementation of this path, so the oracle is this repo's CPU
implementation of docs/SPEC.md — "parity unpinned" with respect to the reference. Tolerance: none;
every comparison is exact equality of the bits (gpu_support.assert_same_bits; NaN-free inputs, the sign of a zero
compared). Special values, subnormals and exact landings: tests/test_stable_bits_gpu.py.
"""
import numpy as np
import pytest

import oracle_lib as O
from gpu_support import (DIFF, DT, DTYPES, NAMES, VISC, S, advect_form, assert_same_bits, check_transport, make,  # noqa: F401
                         march_mode, rand_fields, slab_kw, small_velocity)  # (advect_form, march_mode: fixtures)

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 8, 13, 16, 31, 34]
TRANSPORTS = ["copy", "rccl-self"]  # (gpu_support.make)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_upload_download_roundtrip(N, dtype):
    f = rand_fields(N, dtype, 1)
    with make(N, dtype) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        for n in NAMES:
            assert_same_bits(fs.download(n), f[n], f"roundtrip {n}")
        fs.upload("user2", f["u"])
        assert_same_bits(fs.download("user2"), f["u"], "roundtrip user slot")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", SIZES)
def test_add_source(N, dtype):
    f = rand_fields(N, dtype, 2)
    with make(N, dtype) as fs:
        fs.upload("dens", f["dens"])
        fs.upload("dens0", f["dens0"])
        fs.add_source("dens", "dens0")
        got = fs.download("dens")
    O.add_source(f["dens"], f["dens0"], DT)
    assert_same_bits(got, f["dens"], "add_source")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("b", [0, 1, 2, 3])
@pytest.mark.parametrize("N", [1, 2, 5, 16, 33])
def test_set_bnd(N, b, dtype):
    f = rand_fields(N, dtype, 3)
    with make(N, dtype) as fs:
        fs.upload("u", f["u"])
        fs.set_bnd(b, "u")
        got = fs.download("u")
    O.set_bnd(b, f["u"])
    assert_same_bits(got, f["u"], f"set_bnd b={b}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("b", [0, 1, 2, 3])
@pytest.mark.parametrize("N,K", [(1, 3), (2, 2), (3, 5), (8, 4), (13, 3), (16, 1), (31, 6), (34, 7), (64, 3)])
def test_lin_solve(N, K, b, dtype, march_mode):
    f = rand_fields(N, dtype, 4)
    a, c = 0.37, 1 + 6 * 0.37
    with make(N, dtype) as fs:
        fs.upload("dens", f["dens"])
        fs.upload("dens0", f["dens0"])
        fs.lin_solve(b, "dens", "dens0", a, c, K)
        got = fs.download("dens")
        x0_after = fs.download("dens0")
    want = f["dens"].copy()
    O.lin_solve(b, want, f["dens0"], dtype(a), dtype(c), K)
    assert_same_bits(got, want, f"lin_solve b={b} K={K}")
    assert_same_bits(x0_after, f["dens0"], "lin_solve must not touch x0")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,K,b", [(100, 4, 1), (108, 5, 2), (20, 6, 3), (324, 4, 0), (408, 2, 1), (516, 2, 3),
                                   (100, 9, 2), (44, 11, 3), (324, 8, 1), (200, 7, 0)])
def test_lin_solve_rows_that_straddle_waves(N, K, b, dtype, march_mode):
    """Row widths that are not a power of two, and rows wider than two waves (up to 258 vectors here): the fused
    kernel's overlapped mapping packs the (row pair, vector) items of a plane pair into 60-lane windows, so rows
    start and end anywhere inside a wave."""
    if march_mode == "marching" and N >= 300:
        pytest.skip("above the marching kernel's size threshold 'auto' already is the marching schedule")
    if N >= 500 and dtype == np.float64:
        pytest.skip("512^3 fp64 against the oracle: tests/test_full_size_gpu.py")
    f = rand_fields(N, dtype, 50)
    a, c = 0.21, 1 + 6 * 0.21
    with make(N, dtype) as fs:
        fs.upload("dens", f["dens"])
        fs.upload("dens0", f["dens0"])
        fs.lin_solve(b, "dens", "dens0", a, c, K)
        got = fs.download("dens")
    want = f["dens"].copy()
    O.lin_solve(b, want, f["dens0"], dtype(a), dtype(c), K)
    assert_same_bits(got, want, f"lin_solve N={N} K={K}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_lin_solve_zero_iters_is_noop(dtype):
    f = rand_fields(8, dtype, 5)
    with make(8, dtype) as fs:
        fs.upload("dens", f["dens"])
        fs.upload("dens0", f["dens0"])
        fs.lin_solve(0, "dens", "dens0", 1.0, 6.0, 0)
        assert_same_bits(fs.download("dens"), f["dens"], "K=0")


ADVECT_CASES = [(N, b) for N in (1, 2, 5, 8, 16, 31) for b in (0, 1, 2, 3)] + [(34, 1), (70, 2), (130, 3), (130, 0), (256, 0),
                                                                                 (256, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,b", ADVECT_CASES)
def test_advect(N, b, dtype, advect_form):

    # velocities large enough to hit the clamp at both ends and every fractional position
    f = rand_fields(N, dtype, 6, scale=1.0)
    with make(N, dtype) as fs:
        for n in ("dens", "dens0", "u", "v", "w"):
            fs.upload(n, f[n])
        fs.advect(b, "dens", "dens0", "u", "v", "w")
        got = fs.download("dens")
    want = f["dens"].copy()
    O.advect(b, want, f["dens0"], f["u"], f["v"], f["w"], dtype(DT))
    assert_same_bits(got, want, f"advect b={b}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,b", [(34, 0), (70, 1), (130, 2), (200, 3)])
def test_advect_smooth_flow(N, b, dtype, advect_form):
    """A smooth velocity field (back-traces of up to ~2.5 cells that vary slowly along a row): neighbouring cells land
    in neighbouring cells, the case in which the one-cell-per-lane form takes its i0+1 samples from the next lane —
    with the integer part stepping a few times per row, where it must fall back to its own loads."""
    f = rand_fields(N, dtype, 7, scale=1.0)
    k, j, i = np.meshgrid(*(np.arange(N + 2, dtype=np.float64),) * 3, indexing="ij")
    amp = 2.5 / (DT * N)
    f["u"] = (amp * np.sin(2 * np.pi * i / N + 0.3) * np.cos(2 * np.pi * j / N)).astype(dtype)
    f["v"] = (amp * np.cos(2 * np.pi * (i + k) / N)).astype(dtype)
    f["w"] = (amp * np.sin(2 * np.pi * (j - i) / N + 1.1)).astype(dtype)
    with make(N, dtype) as fs:
        for n in ("dens", "dens0", "u", "v", "w"):
            fs.upload(n, f[n])
        fs.advect(b, "dens", "dens0", "u", "v", "w")
        got = fs.download("dens")
    want = f["dens"].copy()
    O.advect(b, want, f["dens0"], f["u"], f["v"], f["w"], dtype(DT))
    assert_same_bits(got, want, f"advect (smooth flow) N={N} b={b}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["near", "mixed"])
@pytest.mark.parametrize("N,b", [(1, 0), (3, 1), (8, 2), (13, 3), (32, 1), (64, 0), (100, 2), (130, 3)])
def test_advect_short_and_long_backtraces(N, b, mode, dtype, advect_form):
    if advect_form in ("row", "pairs") and N < 32:
        pytest.skip("the one-cell-per-lane forms on tiny grids: test_advect")
    """Back-traces shorter than one cell ('near'), and 'mixed': a few long back-traces (several cells, clamped at the
    walls) scattered into the field. Either way the result must equal the oracle."""
    rng = np.random.RandomState(60 + N)
    f = rand_fields(N, dtype, 61)
    lim = 0.95 / (DT * N)
    for n in ("u", "v", "w"):
        f[n] = rng.uniform(-lim, lim, size=f[n].shape).astype(dtype)
    if mode == "mixed":
        for n in ("u", "v", "w"):
            idx = tuple(rng.randint(0, N + 2, size=(3, max(1, N // 2))))
            f[n][idx] = dtype(rng.choice([-4.0, 3.0]))
    with make(N, dtype) as fs:
        for n in ("dens", "dens0", "u", "v", "w"):
            fs.upload(n, f[n])
        fs.advect(b, "dens", "dens0", "u", "v", "w")
        got = fs.download("dens")
    want = f["dens"].copy()
    O.advect(b, want, f["dens0"], f["u"], f["v"], f["w"], dtype(DT))
    assert_same_bits(got, want, f"advect({mode}) b={b}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,K", [(1, 2), (3, 3), (8, 4), (17, 5), (32, 6), (36, 9), (20, 12), (100, 8)])
def test_project(N, K, dtype, march_mode):
    f = rand_fields(N, dtype, 7)
    with make(N, dtype, K=K) as fs:
        for n in ("u", "v", "w", "u0", "v0"):
            fs.upload(n, f[n])
        fs.project("u", "v", "w", "u0", "v0")
        got = {n: fs.download(n) for n in ("u", "v", "w", "u0", "v0")}
    O.project(f["u"], f["v"], f["w"], f["u0"], f["v0"], K)
    for n in ("u", "v", "w", "u0", "v0"):
        assert_same_bits(got[n], f[n], f"project {n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,K,steps", [(2, 3, 2), (7, 4, 2), (16, 5, 3), (32, 10, 1), (34, 4, 2), (64, 6, 1)])
def test_full_steps(N, K, steps, dtype, march_mode):
    f = rand_fields(N, dtype, 8)
    src = {n: f[n].copy() for n in ("u0", "v0", "w0", "dens0")}
    with make(N, dtype, K=K) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        for s in range(steps):
            if s > 0:
                for n in src:
                    fs.upload(n, src[n])
            fs.vel_step()
            fs.dens_step()
        fs.sync()
        got = {n: fs.download(n) for n in NAMES}
    for s in range(steps):
        if s > 0:
            for n in src:
                f[n][...] = src[n]
        O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in NAMES:
        assert_same_bits(got[n], f[n], f"after {steps} steps: {n}")


# ---- slab decomposition on ONE device: P logical slabs, device-to-device halo transport ----------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("transport", TRANSPORTS)
@pytest.mark.parametrize("N,P", [(2, 2), (4, 4), (8, 2), (8, 8), (12, 3), (16, 4), (32, 2), (34, 17)])
def test_slabs_full_step_bit_identical(N, P, transport, dtype):
    K = 5
    f = small_velocity(rand_fields(N, dtype, 9), N, dtype)
    with make(N, dtype, K=K, **slab_kw(transport, P)) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        fs.vel_step()
        fs.dens_step()
        fs.sync()
        check_transport(fs, transport, P)
        got = {n: fs.download(n) for n in NAMES}
    O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in NAMES:
        assert_same_bits(got[n], f[n], f"P={P}: {n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("transport", TRANSPORTS)
@pytest.mark.parametrize("N,P,K,steps", [(64, 2, 7, 2), (64, 8, 6, 1), (48, 4, 4, 2), (128, 4, 5, 1),
                                         # solves that end in (or consist of) a single sweep or a pair on slabs deep
                                         # enough for three / four ghost planes under "marching"
                                         (128, 4, 1, 1), (128, 4, 2, 1), (96, 4, 9, 1), (128, 2, 13, 1), (96, 2, 3, 2)])
def test_slabs_fused_pairs_two_ghost_planes(N, P, K, steps, transport, dtype, march_mode):
    """N % vector width == 0 and >= 2 planes per slab: sweep pairs are fused across slab boundaries (two ghost
    planes, one exchange per pair, div recomputed on the first ghost plane). Must still equal the oracle."""
    f = small_velocity(rand_fields(N, dtype, 21), N, dtype)
    src = {n: f[n].copy() for n in ("u0", "v0", "w0", "dens0")}
    with make(N, dtype, K=K, **slab_kw(transport, P)) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        for s in range(steps):
            if s > 0:
                for n in src:
                    fs.upload(n, src[n])
            fs.vel_step()
            fs.dens_step()
        fs.sync()
        check_transport(fs, transport, P)
        got = {n: fs.download(n) for n in NAMES}
    for s in range(steps):
        if s > 0:
            for n in src:
                f[n][...] = src[n]
        O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in NAMES:
        assert_same_bits(got[n], f[n], f"P={P} fused: {n}")


@pytest.mark.parametrize("transport", TRANSPORTS)
@pytest.mark.parametrize("prio", ["0", "1"])
@pytest.mark.parametrize("N,P,K", [(128, 2, 6), (128, 8, 5), (192, 4, 4), (256, 8, 3)])
def test_slabs_stress_against_single_slab(N, P, K, prio, transport, monkeypatch):
    """Timing-sensitive check of the halo overlap: large interior launches run concurrently with the exchange.
    The decomposed run must equal the single-slab GPU run bit for bit, with the halo stream at normal and at
    highest priority (the latter exposed a missing dependency during development), repeated."""
    dtype = np.float32
    monkeypatch.setenv("SF_HALO_PRIO", prio)
    f = small_velocity(rand_fields(N, dtype, 40 + P), N, dtype)

    def run(nslabs):
        with make(N, dtype, K=K, **slab_kw(transport, nslabs)) as fs:
            for n in NAMES:
                fs.upload(n, f[n])
            for _ in range(2):
                fs.copy_field("user0", "u")  # extra traffic on the compute stream between steps
                fs.vel_step()
                fs.dens_step()
            fs.sync()
            check_transport(fs, transport, nslabs)
            return {n: fs.download(n) for n in ("u", "v", "w", "dens")}

    want = run(1)
    for rep in range(2):
        got = run(P)
        for n in want:
            assert_same_bits(got[n], want[n], f"N={N} P={P} prio={prio} rep={rep}: {n}")


@pytest.mark.parametrize("N,P,K,trap", [(128, 2, 20, "5"), (128, 4, 20, "3"), (160, 4, 12, "10"), (320, 2, 20, "5"),
                                        (128, 2, 20, "0"), (64, 2, 9, "4"),
                                        # launches of different depth inside one trapezoid block (4 then 3, 4 3 2, ...)
                                        (128, 2, 7, "5"), (128, 2, 9, "5"), (96, 2, 11, "8"), (160, 2, 23, "8")])
@pytest.mark.parametrize("transport", TRANSPORTS)
def test_slabs_trapezoid_schedule(N, P, K, trap, transport, monkeypatch, march_mode):
    """lin_solve on a decomposed grid: the boundary launch grows by two planes per pair so that consecutive interior
    launches need no cross-stream wait (SF_TRAP pairs per block; 0 = off). Long solves (several blocks, a resync in
    between, odd K, a row width that takes the overlapped mapping) must equal the single-slab GPU run bit for bit."""
    dtype = np.float32
    monkeypatch.setenv("SF_TRAP", trap)
    f = small_velocity(rand_fields(N, dtype, 70 + P), N, dtype)

    def run(nslabs):
        with make(N, dtype, K=K, **slab_kw(transport, nslabs)) as fs:
            for n in NAMES:
                fs.upload(n, f[n])
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            return {n: fs.download(n) for n in ("u", "v", "w", "dens")}

    want = run(1)
    for rep in range(2):
        got = run(P)
        for n in want:
            assert_same_bits(got[n], want[n], f"N={N} P={P} K={K} trap={trap} rep={rep}: {n}")


@pytest.mark.parametrize("transport", TRANSPORTS)
@pytest.mark.parametrize("N,P,K", [(128, 2, 8), (96, 4, 5), (64, 8, 4), (160, 2, 20)])
def test_slabs_halo_on_the_boundary_stream(N, P, K, transport, monkeypatch, march_mode):
    """One slab per process issues its halo messages on the boundary stream (no cross-stream hand-over in the chain
    boundary launch -> message -> next boundary launch). SF_HALO_STREAM=2 applies the same stream sharing to the
    logical slabs of one process, where the result can be checked: bit-identical to the single-slab run, with bound
    sources (folded add_source + ghost-plane right-hand side on that stream) and without."""
    dtype = np.float32
    monkeypatch.setenv("SF_HALO_STREAM", "2")
    f = small_velocity(rand_fields(N, dtype, 80 + P), N, dtype)

    def run(nslabs, bound):
        with make(N, dtype, K=K, **slab_kw(transport, nslabs)) as fs:
            for n in NAMES:
                fs.upload(n, f[n])
            if bound:
                for slot, n in (("user0", "u0"), ("user1", "v0"), ("user2", "w0"), ("user3", "dens0")):
                    fs.upload(slot, f[n])
                fs.bind_sources("user0", "user1", "user2", "user3")
            for _ in range(2):
                fs.vel_step()
                fs.dens_step()
            fs.sync()
            check_transport(fs, transport, nslabs)
            return {n: fs.download(n) for n in ("u", "v", "w", "dens")}

    for bound in (False, True):
        want = run(1, bound)
        got = run(P, bound)
        for n in want:
            assert_same_bits(got[n], want[n], f"N={N} P={P} K={K} bound={bound}: {n}")


@pytest.mark.parametrize("split", ["0", "2"])
def test_diffuse_fields_together_or_one_by_one(split, monkeypatch):
    """SF_SPLIT_FIELDS: u, v, w diffused in one three-field launch per pair or one field after the other."""
    N, K, dtype = 40, 6, np.float32
    monkeypatch.setenv("SF_SPLIT_FIELDS", split)
    f = small_velocity(rand_fields(N, dtype, 91), N, dtype)
    with make(N, dtype, K=K) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        fs.vel_step()
        fs.dens_step()
        fs.sync()
        got = {n: fs.download(n) for n in NAMES}
    O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in NAMES:
        assert_same_bits(got[n], f[n], f"split={split}: {n}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N,K,bound", [(48, 8, True), (66, 12, True), (48, 8, False), (34, 20, True)])
def test_diffuse_fields_as_one_marching_grid(N, K, bound, dtype, monkeypatch):
    """u, v, w of a diffusion as ONE grid of the four-sweep marching kernel (round 3; by default only on undecomposed
    grids of 200^3..550^3, where tests/test_full_size_gpu.py covers it at 256^3): SF_SPLIT_FIELDS=0 applies the rule at
    every size. K a multiple of four: folded-source first pass over the three fields (bound sources) or one first pass
    per field (caller data), then plain passes over the three fields, two steps, against the oracle."""
    monkeypatch.setenv("SF_SPLIT_FIELDS", "0")
    monkeypatch.setenv("SF_MARCH_MINCELLS_K", "10")
    monkeypatch.setenv("SF_MARCH_MINP", "4")
    f = small_velocity(rand_fields(N, dtype, 17 + N + K), N, dtype)
    src = {n: f[n].copy() for n in ("u0", "v0", "w0", "dens0")}
    with make(N, dtype, K=K) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        if bound:
            for slot, n in (("user0", "u0"), ("user1", "v0"), ("user2", "w0"), ("user3", "dens0")):
                fs.upload(slot, src[n])
            fs.bind_sources("user0", "user1", "user2", "user3")
        for step in range(2):
            if not bound and step:
                for n in src:
                    fs.upload(n, src[n])
            fs.vel_step()
            fs.dens_step()
        fs.sync()
        got = {n: fs.download(n) for n in ("u", "v", "w", "dens")}
    for _ in range(2):
        for n in src:
            f[n][...] = src[n]
        O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in got:
        assert_same_bits(got[n], f[n], f"one grid N={N} K={K} bound={bound}: {n}")


def test_loopback_rank_share_context():
    """SF_FLAG_LOOPBACK_HALO (measurement aid): rank 1 of 4 without a communicator; the values next to the slab faces are
    meaningless by construction, so this only checks that the context works, stays finite and reports the slab it
    would own."""
    N = 32
    with S().FluidSolver(N, dtype="f32", iters=4, rank=1, nranks=4, flags=1) as fs:
        assert fs.owned_planes() == (9, 17)
        kb, ke = fs.stored_planes()
        z = np.zeros((ke - kb, N + 2, N + 2), np.float32)
        for n in NAMES:
            fs.upload_planes(n, kb, z + (0.25 if n == "dens" else 0.0))
        fs.vel_step()
        fs.dens_step()
        fs.sync()
        d = fs.download_planes("dens", 9, 17)
        assert np.isfinite(d).all()
        assert fs.schedule_info()["measured"] is False  # slab too thin for a trapezoid block: nothing to measure
    # a slab thick enough: sf_create times the candidate schedules and leaves the fields zero
    with S().FluidSolver(96, dtype="f32", iters=4, rank=0, nranks=2, flags=1) as fs:
        info = fs.schedule_info()
        import os

        if "SF_TRAP" not in os.environ and os.environ.get("SF_AUTOTUNE", "1") != "0":  # either switches it off
            assert info["measured"] is True and info["trapezoid_pairs"] in (0, 2, 5)
        if "SF_SPLIT_FIELDS" in os.environ or not info["measured"]:
            info = dict(info, fields_measured=True, fields_per_launch=1)  # nothing to assert below
        kb, ke = fs.owned_planes()
        assert info["fields_measured"] is True and info["fields_per_launch"] in (1, 3)
        for n in ("dens", "dens0", "u", "v0", "w"):
            assert not fs.download_planes(n, kb, ke).any(), f"{n} must still be zero after the schedule measurement"


def test_upload_planes_fills_all_ghosts():
    """A rank that fills exactly sf_stored_planes() with sf_upload_planes gets the same state as sf_upload."""
    N, dtype, P = 16, np.float32, 4
    f = small_velocity(rand_fields(N, dtype, 22), N, dtype)
    out = []
    for mode in ("full", "planes"):
        with make(N, dtype, K=4, nslabs_local=P) as fs:
            kb, ke = fs.stored_planes()
            assert (kb, ke) == (0, N + 2)
            for n in NAMES:
                if mode == "full":
                    fs.upload(n, f[n])
                else:
                    fs.upload_planes(n, kb, f[n][kb:ke])
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            out.append({n: fs.download(n) for n in NAMES})
    for n in NAMES:
        assert_same_bits(out[1][n], out[0][n], n)


@pytest.mark.parametrize("P", [2, 4])
def test_slabs_each_operator(P):
    N, dtype, K = 16, np.float32, 4
    f = small_velocity(rand_fields(N, dtype, 10), N, dtype)
    with make(N, dtype, K=K, nslabs_local=P) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        fs.set_bnd(2, "w0")
        fs.lin_solve(1, "dens", "dens0", 0.5, 4.0, 3)
        fs.advect(3, "u0", "v0", "u", "v", "w")
        fs.sync()
        got = {n: fs.download(n) for n in ("w0", "dens", "u0")}
    O.set_bnd(2, f["w0"])
    O.lin_solve(1, f["dens"], f["dens0"], dtype(0.5), dtype(4.0), 3)
    O.advect(3, f["u0"], f["v0"], f["u"], f["v"], f["w"], dtype(DT))
    for n in got:
        assert_same_bits(got[n], f[n], f"P={P}: {n}")


def test_slabs_halo_exceeded_is_reported():
    N, dtype = 16, np.float32
    f = rand_fields(N, dtype, 11)
    f["w"][...] = 3.0  # dt*N*w = 4.8 planes
    Sx = S()
    with make(N, dtype, nslabs_local=4) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        fs.advect(0, "dens", "dens0", "u", "v", "w")
        with pytest.raises(Sx.SfError) as e:
            fs.sync()
        assert e.value.status == Sx.SF_ERR_HALO_EXCEEDED
        fs.sync()  # flag is cleared once reported


def test_download_planes_and_owned_range():
    N, dtype = 8, np.float32
    f = rand_fields(N, dtype, 12)
    with make(N, dtype, nslabs_local=2) as fs:
        fs.upload("dens", f["dens"])
        assert fs.owned_planes() == (1, N + 1)
        got = fs.download_planes("dens", 3, 7)
    assert_same_bits(got, f["dens"][3:7], "download_planes")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", [4, 16, 33])
def test_tracers(N, dtype):
    rng = np.random.RandomState(31)
    f = rand_fields(N, dtype, 30, scale=0.5)
    n = 1000
    pos = (rng.uniform(-1.0, N + 2.0, size=(n, 3))).astype(dtype)  # some start outside the box: they get clamped
    with make(N, dtype) as fs:
        for k in ("u", "v", "w", "dens"):
            fs.upload(k, f[k])
        fs.tracers_set(pos)
        for _ in range(3):
            fs.tracers_advect()
        got_pos, got_d, got_s = fs.tracers_get()
    want = pos.copy()
    for _ in range(3):
        O.tracers_advect(want, f["u"], f["v"], f["w"], dtype(DT))
    want_d, want_s = O.tracers_sample(want, f["dens"], f["u"], f["v"], f["w"])
    assert_same_bits(got_pos, want, "tracer positions")
    assert_same_bits(got_d, want_d, "tracer density sample")
    assert_same_bits(got_s, want_s, "tracer speed sample")


def test_tracers_survive_the_copy_bandwidth_probe():
    """sf_tracers_set -> sf_measure_copy_bandwidth (two sizes: the probe re-allocates its buffers) -> sf_tracers_advect
    -> sf_tracers_get. The probe once freed the tracer arrays (a mis-pasted block): kernels then ran on freed memory
    that the probe's own buffers could re-use. The tracers must come out exactly as the oracle's."""
    N, dtype = 16, np.float32
    rng = np.random.RandomState(5)
    f = rand_fields(N, dtype, 33, scale=0.5)
    n = 50000
    pos = rng.uniform(0.5, N + 0.5, size=(n, 3)).astype(dtype)
    with make(N, dtype) as fs:
        for k in ("u", "v", "w", "dens"):
            fs.upload(k, f[k])
        fs.tracers_set(pos)
        fs.tracers_advect()
        assert fs.copy_bandwidth_gbps(8 << 20, 2) > 0
        assert fs.copy_bandwidth_gbps(32 << 20, 2) > 0
        fs.tracers_advect()
        got_pos, got_d, got_s = fs.tracers_get()
        fs.tracers_set(pos[:100])  # re-setting frees the old arrays exactly once
        assert fs.copy_bandwidth_gbps(8 << 20, 1) > 0
        fs.tracers_advect()
        got2, _, _ = fs.tracers_get()
    want = pos.copy()
    for _ in range(2):
        O.tracers_advect(want, f["u"], f["v"], f["w"], dtype(DT))
    want_d, want_s = O.tracers_sample(want, f["dens"], f["u"], f["v"], f["w"])
    assert_same_bits(got_pos, want, "tracer positions after the bandwidth probe")
    assert_same_bits(got_d, want_d, "tracer density sample after the bandwidth probe")
    assert_same_bits(got_s, want_s, "tracer speed sample after the bandwidth probe")
    want2 = pos[:100].copy()
    O.tracers_advect(want2, f["u"], f["v"], f["w"], dtype(DT))
    assert_same_bits(got2, want2, "re-set tracers")


@pytest.mark.parametrize("P", [1, 4])
def test_snapshot_is_a_consistent_async_copy(P):
    """sf_snapshot + sf_snapshot_read (from another thread, while the owner keeps stepping) returns the state at
    the time of the snapshot."""
    import threading

    N, dtype, K = 32, np.float32, 4
    f = small_velocity(rand_fields(N, dtype, 32), N, dtype)
    with make(N, dtype, K=K, nslabs_local=P) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        fs.vel_step()
        fs.dens_step()
        fs.snapshot(["dens", "u", "v", "w"])
        result = {}

        def reader():
            for q, n in enumerate(("dens", "u", "v", "w")):
                result[n] = fs.snapshot_read(q)
            result["dens[5:19]"] = fs.snapshot_read_planes(0, 5, 19)  # a plane range across slab boundaries

        th = threading.Thread(target=reader)
        th.start()
        for _ in range(3):  # keep the device busy with later steps
            fs.vel_step()
            fs.dens_step()
        th.join()
        fs.sync()
    O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in ("dens", "u", "v", "w"):
        assert_same_bits(result[n], f[n], f"snapshot {n}")
    assert_same_bits(result["dens[5:19]"], f["dens"][5:19], "snapshot plane range")


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("N,K,dtype,P", [(24, 5, np.float32, 1), (24, 5, np.float32, 2), (40, 2, np.float32, 1),
                                          (40, 3, np.float64, 1), (100, 6, np.float32, 1), (64, 4, np.float64, 1),
                                          (128, 7, np.float32, 1), (136, 4, np.float32, 1), (8, 4, np.float32, 1),
                                          (6, 1, np.float32, 1), (256, 4, np.float32, 1), (64, 6, np.float32, 4),
                                          (128, 20, np.float32, 2), (160, 6, np.float32, 4), (64, 5, np.float64, 2),
                                          (16, 4, np.float32, 8), (16, 4, np.float32, 4), (36, 9, np.float32, 1),
                                          (52, 12, np.float64, 1), (100, 8, np.float32, 1), (200, 7, np.float32, 1)])
def test_bound_sources(N, K, dtype, P, fuse, monkeypatch, march_mode):
    """sf_bind_sources == copying the user slots into u0/v0/w0/dens0 before every step, bit for bit — with add_source
    folded into the first sweep pair of diffuse (SF_FUSE_SRC=1, single slab) and as a separate pass."""
    monkeypatch.setenv("SF_FUSE_SRC", fuse)
    steps = 3 if N <= 64 else 2
    f = small_velocity(rand_fields(N, dtype, 70), N, dtype)
    src = {"u0": f["u0"].copy(), "v0": f["v0"].copy(), "w0": f["w0"].copy(), "dens0": f["dens0"].copy()}
    with make(N, dtype, K=K, nslabs_local=P) as fs:
        for n in ("u", "v", "w", "dens"):
            fs.upload(n, f[n])
        for slot, n in (("user0", "u0"), ("user1", "v0"), ("user2", "w0"), ("user3", "dens0")):
            fs.upload(slot, src[n])
        fs.bind_sources("user0", "user1", "user2", "user3")
        for _ in range(steps):
            fs.vel_step()
            fs.dens_step()
        fs.sync()
        got = {n: fs.download(n) for n in NAMES}
        assert_same_bits(fs.download("user1"), src["v0"], "bound source slot must stay untouched")
    for _ in range(steps):
        for n in src:
            f[n][...] = src[n]
        O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in NAMES:
        assert_same_bits(got[n], f[n], f"bound sources N={N} K={K} P={P} fuse={fuse}: {n}")


def test_graph_replay_matches(monkeypatch):
    """SF_GRAPH=1: steps captured into hipGraphs and replayed (several buffer arrangements, odd K) equal the oracle."""
    monkeypatch.setenv("SF_GRAPH", "1")
    N, dtype, K = 20, np.float32, 5
    f = small_velocity(rand_fields(N, dtype, 80), N, dtype)
    src = {n: f[n].copy() for n in ("u0", "v0", "w0", "dens0")}
    with make(N, dtype, K=K) as fs:
        for n in ("u", "v", "w", "dens"):
            fs.upload(n, f[n])
        for slot, n in (("user0", "u0"), ("user1", "v0"), ("user2", "w0"), ("user3", "dens0")):
            fs.upload(slot, src[n])
        fs.bind_sources("user0", "user1", "user2", "user3")
        for _ in range(6):
            fs.vel_step()
            fs.dens_step()
        fs.sync()
        got = {n: fs.download(n) for n in ("u", "v", "w", "dens")}
    for _ in range(6):
        for n in src:
            f[n][...] = src[n]
        O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in got:
        assert_same_bits(got[n], f[n], f"graph replay: {n}")


def test_invalid_arguments_are_rejected():
    Sx = S()
    with pytest.raises(Sx.SfError):
        Sx.FluidSolver(10, nslabs_local=3)  # 10 % 3 != 0
    with make(8, np.float32) as fs:
        with pytest.raises(Sx.SfError):
            fs.lin_solve(0, "dens", "dens", 1, 6, 1)
        with pytest.raises(Sx.SfError):
            fs.set_bnd(7, "dens")
        with pytest.raises(Sx.SfError):
            fs.advect(0, "dens", "dens0", "dens", "v", "w")


# ---- size-independent properties at BASELINE.json's sizes (the oracle is too slow there) ---------

@pytest.mark.parametrize("N,dtype", [(256, np.float32), (512, np.float64)], ids=["256-f32", "512-f64"])
def test_large_properties(N, dtype):
    """Size-independent properties at configs[1] and configs[4] of BASELINE.json (grid and precision). The bit-exact
    comparisons with the oracle at these sizes, and at configs[2] (512^3 fp32), are in tests/test_full_size_gpu.py."""
    K = 20
    rng = np.random.RandomState(13)
    with make(N, dtype, K=K) as fs:
        # (1) all-zero state and sources stay zero
        fs.vel_step()
        fs.dens_step()
        fs.sync()
        for n in ("u", "v", "w", "dens"):
            assert not fs.download(n).any()
        # (2) uniform density, zero velocity, zero diffusivity (a = 0: each sweep returns x0 exactly):
        # unchanged by dens_step
        fs.set_coefficients(DT, 0.0, 0.0)
        fs.fill("dens", 0.75)
        fs.fill("dens0", 0.0)
        fs.dens_step()
        fs.sync()
        d = fs.download("dens")
        assert np.all(d == dtype(0.75))
        fs.set_coefficients(DT, DIFF, VISC)
        # (3) Jacobi fixed point: x0 := c*x - a*sum(x_nb) makes x a fixed point up to rounding; instead
        # use linearity-free exact check: zero neighbours. x = 0, x0 = r  ->  one sweep gives r*inv exactly.
        r = rng.standard_normal((N + 2,) * 3).astype(dtype)
        fs.upload("dens0", r)
        fs.fill("dens", 0.0)
        a, c = 0.25, 2.5
        fs.lin_solve(0, "dens", "dens0", a, c, 1)
        got = fs.download("dens")
        inv = dtype(1) / dtype(c)
        want = (r[1:-1, 1:-1, 1:-1] + dtype(a) * dtype(0)) * inv
        assert np.array_equal(got[1:-1, 1:-1, 1:-1], want)
        # shell = copy of the adjacent interior (b = 0)
        assert np.array_equal(got[0, 1:-1, 1:-1], got[1, 1:-1, 1:-1])
        assert np.array_equal(got[1:-1, -1, 1:-1], got[1:-1, -2, 1:-1])
        assert np.array_equal(got[1:-1, 1:-1, 0], got[1:-1, 1:-1, 1])
        # (4) advect with zero velocity is the identity on the interior
        fs.fill("u", 0.0)
        fs.fill("v", 0.0)
        fs.fill("w", 0.0)
        fs.upload("dens0", r)
        fs.advect(0, "dens", "dens0", "u", "v", "w")
        got = fs.download("dens")
        assert np.array_equal(got[1:-1, 1:-1, 1:-1], r[1:-1, 1:-1, 1:-1])
        # (5) slab-decomposed run equals the single-slab run bit for bit
    f = small_velocity(rand_fields(N, dtype, 14), N, dtype)
    out = []
    for P in (1, 4):
        with make(N, dtype, K=4, nslabs_local=P) as fs:
            for n in NAMES:
                fs.upload(n, f[n])
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            out.append({n: fs.download(n) for n in ("u", "v", "w", "dens")})
    for n in out[0]:
        assert_same_bits(out[1][n], out[0][n], f"{N}^3 P=4 vs P=1: {n}")
    # (6) mirror symmetry of a centred source (x -> N+1-x) is preserved by dens diffusion
    with make(N, dtype, K=6) as fs:
        src = np.zeros((N + 2,) * 3, dtype)
        src[N // 2:N // 2 + 2, N // 2:N // 2 + 2, N // 2:N // 2 + 2] = 100
        fs.upload("dens0", src)
        fs.dens_step()
        fs.sync()
        d = fs.download("dens")
        assert d.max() > 0
        assert np.array_equal(d, d[::-1, :, :]) and np.array_equal(d, d[:, ::-1, :]) and np.array_equal(d, d[:, :, ::-1])


@pytest.mark.parametrize("N,dtype", [(1024, np.float32), (512, np.float64)], ids=["config4-1024-f32", "config5-512-f64"])
def test_decomposed_configs_eight_slabs_equal_one(N, dtype):
    """configs[3] and configs[4] of BASELINE.json: the 1024^3 fp32 / 512^3 fp64 grids cut into eight k-slabs (logical
    slabs on one GPU: same kernels, ghost planes and exchange schedule as eight ranks), with the ghost planes moved by
    the copy kernel and by RCCL send/recv through a single-rank communicator (the transport of the eight-rank run).
    lin_solve on rows of 256 vectors (fused pairs through the overlapped mapping, two ghost planes) and one full
    step must equal the undecomposed run bit for bit."""
    K = 4
    rng = np.random.RandomState(31)
    plane = rng.standard_normal((1, N + 2, N + 2)).astype(dtype)
    res = []
    for P, transport in ((1, "copy"), (8, "copy"), (8, "rccl-self")):
        with make(N, dtype, K=K, **slab_kw(transport, P)) as fs:
            for k in range(N + 2):
                fs.upload_planes("dens", k, plane * dtype(1 + 0.001 * k))
                fs.upload_planes("dens0", k, plane * dtype(0.5 - 0.0005 * k))
            fs.lin_solve(0, "dens", "dens0", 0.3, 2.8, K)
            fs.sync()
            check_transport(fs, transport, P)
            if transport == "rccl-self":  # sf_create measured the launch schedule over the communicator
                assert fs.schedule_info()["measured"]
            res.append(fs.download("dens"))
    assert np.isfinite(res[0]).all() and res[0].std() > 0
    assert_same_bits(res[1], res[0], f"{N}^3 lin_solve, 8 slabs (copy) vs 1")
    assert_same_bits(res[2], res[0], f"{N}^3 lin_solve, 8 slabs (rccl-self) vs 1")
    del res

    # one full vel_step + dens_step (K = 2) on the same grid; velocities small enough for the one-plane back-trace rule
    out = []
    for P, transport in ((1, "copy"), (8, "copy"), (8, "rccl-self")):
        with make(N, dtype, K=2, **slab_kw(transport, P)) as fs:
            for q, n in enumerate(NAMES):
                scale = dtype(0.25 if n.startswith("dens") else 2.0 / N)
                for k in range(N + 2):
                    fs.upload_planes(n, k, plane * (scale * dtype(1 + 0.0007 * ((k + 37 * q) % 101))))
            fs.vel_step()
            fs.dens_step()
            fs.sync()
            check_transport(fs, transport, P)
            out.append({n: fs.download(n) for n in ("u", "w", "dens")})
    for n in out[0]:
        assert np.isfinite(out[0][n]).all()
        assert_same_bits(out[1][n], out[0][n], f"{N}^3 full step, 8 slabs (copy) vs 1: {n}")
        assert_same_bits(out[2][n], out[0][n], f"{N}^3 full step, 8 slabs (rccl-self) vs 1: {n}")


def test_driver_frame_equals_config1_golden(tmp_path):
    """End to end through the C++ driver: config 1 (32^3, K = 10, one step) run on the GPU and written by the
    driver's asynchronous writer must be byte-identical to the frame the CPU oracle + reference writer produced
    (tests/golden/config1_frame.json)."""
    import hashlib
    import json
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gold = json.load(open(os.path.join(root, "tests", "golden", "config1_frame.json")))
    exe = os.path.join(root, "fluidsolvergpu_amd", "sf_driver")
    for flag, key in (("--binary", "binary"), (None, "ascii")):
        cmd = [exe, "--n", "32", "--iters", "10", "--steps", "1", "--every", "1", "--plumbing", "--out", str(tmp_path)]
        if flag:
            cmd.append(flag)
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "t= 0" in out.stdout and "Elapsed kernel time:" in out.stdout
        data = open(tmp_path / "anim_s0.vtk", "rb").read()
        assert len(data) == gold[key]["bytes"]
        assert hashlib.sha256(data).hexdigest() == gold[key]["sha256"]


def test_driver_slab_frames_equal_the_single_slab_frame(tmp_path):
    """The C++ driver with several logical slabs (per-slab inputs through sf_upload_planes, frame buffers sized to the
    owned planes, plane-ranged snapshot reads) writes the same bytes as with one slab, synchronously and through the
    writer thread."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "fluidsolvergpu_amd", "sf_driver")
    frames = {}
    for tag, extra in (("one", []), ("four", ["--slabs", "4"]), ("four-sync", ["--slabs", "4", "--sync-output"])):
        out_dir = tmp_path / tag
        cmd = [exe, "--n", "48", "--iters", "6", "--steps", "3", "--every", "2", "--binary", "--quiet", "--out",
               str(out_dir)] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        frames[tag] = [open(out_dir / f"anim_s{q}.vtk", "rb").read() for q in (0, 1)]
    assert frames["four"] == frames["one"] and frames["four-sync"] == frames["one"]


def test_driver_rank_share_of_config4_fits_in_host_memory(tmp_path):
    """One rank's share of BASELINE.json configs[3] (1024^3 over 8 ranks) through the C++ driver: rank 3 of 8 in
    loopback mode on the one GPU (same slab, buffers, launches and frame file as in the eight-rank run; halo messages
    are local copies). The driver must hold only its own planes on the host: peak resident memory of the process
    below 8 GB (it was ~52 GB per rank when every rank materialised the global arrays), and the rectilinear slab
    frame must have the size of 128 planes."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "fluidsolvergpu_amd", "sf_driver")

    # the driver runs as the ONLY child of a small wrapper, whose RUSAGE_CHILDREN high-water mark is then the driver's
    # own (this process's RUSAGE_CHILDREN is a maximum over every child any earlier test has waited for)
    wrapper = ("import resource, subprocess, sys; r = subprocess.run(sys.argv[1:]); "
               "print('MAXRSS_KB', resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss); sys.exit(r.returncode)")
    cmd = [sys.executable, "-c", wrapper, exe, "--n", "1024", "--iters", "4", "--steps", "1", "--every", "1", "--binary",
           "--quiet", "--loopback", "--rank", "3", "--world", "8", "--out", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    peak_kb = int([ln for ln in out.stdout.splitlines() if ln.startswith("MAXRSS_KB")][-1].split()[1])
    assert peak_kb < 8 * 1024 * 1024, f"driver peak RSS {peak_kb / 1048576:.1f} GiB"
    size = os.path.getsize(tmp_path / "anim_s_GPU3_0.vtk")
    cells = 1024 * 1024 * 128
    assert cells * 16 < size < cells * 16 + 20000  # density + 3 velocity components, 4 bytes each, plus headers
    os.remove(tmp_path / "anim_s_GPU3_0.vtk")


def _random_cases(n, seed=1234):
    rng = np.random.RandomState(seed)
    out = []
    for q in range(n):
        N = int(rng.choice([1, 2, 3, 4, 6, 7, 8, 10, 12, 15, 16, 20, 24, 28, 33, 36, 40, 48, 52, 60, 64, 68, 72]))
        divs = [d for d in range(1, N + 1) if N % d == 0 and d <= 12]
        P = int(rng.choice(divs))
        K = int(rng.randint(0, 8))
        steps = int(rng.randint(1, 3))
        dtype = np.float32 if rng.rand() < 0.6 else np.float64
        out.append((N, P, K, steps, dtype, int(rng.randint(0, 10 ** 6))))
    return out


@pytest.mark.parametrize("case", _random_cases(36), ids=lambda c: f"N{c[0]}-P{c[1]}-K{c[2]}-s{c[3]}-{'f32' if c[4] == np.float32 else 'f64'}")
def test_randomised_full_steps(case, march_mode):
    """Seeded random sweep over grid size, slab count, iteration count (incl. 0 and odd), steps and dtype."""
    N, P, K, steps, dtype, seed = case
    f = small_velocity(rand_fields(N, dtype, seed), N, dtype)
    src = {n: f[n].copy() for n in ("u0", "v0", "w0", "dens0")}
    with make(N, dtype, K=K, nslabs_local=P) as fs:
        for n in NAMES:
            fs.upload(n, f[n])
        for s in range(steps):
            if s > 0 and s % 2 == 1:
                for n in src:
                    fs.upload(n, src[n])
            fs.vel_step()
            fs.dens_step()
        fs.sync()
        got = {n: fs.download(n) for n in NAMES}
    for s in range(steps):
        if s > 0 and s % 2 == 1:
            for n in src:
                f[n][...] = src[n]
        O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in NAMES:
        assert_same_bits(got[n], f[n], f"{case[:4]}: {n}")


def test_hundred_steps_benchmark_inputs():
    """BASELINE.json configs[1] shape at a size the oracle finishes in seconds: 100 steps of the benchmark inputs
    (docs/SPEC.md §5) with bound sources, K = 20 — still bit-identical after 100 steps. For scale: the fp32 and fp64
    oracles differ by 2.4e-7 (velocity) / 2.9e-5 (density) after 100 steps at 64^3 (tools/precision_report.py)."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import analytic_planes

    N, K, dtype, steps = 48, 20, np.float32, 100
    a = analytic_planes(N, 0, N + 2, DT, dtype)
    f = {"u": a["u"], "v": a["v"], "w": a["w"], "dens": a["dens"]}
    for b, n in ((1, "u"), (2, "v"), (3, "w"), (0, "dens")):
        O.set_bnd(b, f[n])
    with make(N, dtype, K=K) as fs:
        for n in ("u", "v", "w", "dens"):
            fs.upload(n, f[n])
        for slot, n in (("user0", "su"), ("user1", "sv"), ("user2", "sw"), ("user3", "sd")):
            fs.upload(slot, a[n])
        fs.bind_sources("user0", "user1", "user2", "user3")
        for _ in range(steps):
            fs.vel_step()
            fs.dens_step()
        fs.sync()
        got = {n: fs.download(n) for n in ("u", "v", "w", "dens")}
    for _ in range(steps):
        f.update({"u0": a["su"].copy(), "v0": a["sv"].copy(), "w0": a["sw"].copy(), "dens0": a["sd"].copy()})
        O.step(N, f, dtype(DT), dtype(DIFF), dtype(VISC), K)
    for n in got:
        assert_same_bits(got[n], f[n], f"100 steps: {n}")
    assert np.isfinite(got["dens"]).all() and got["dens"].max() > 1.0
