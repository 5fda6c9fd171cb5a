"""Reductions and diagnostics on the GPU (docs/SPEC.md §10): sf_reduce and sf_diagnostics_get through libsfgpu.so
against the numpy reference (tests/diagnostics_ref.py). Every comparison is exact equality of the bits of the doubles
(a NaN sum equals any NaN: its payload is unspecified), for every decomposition and transport of the case table."""
import os
import re
import subprocess

import numpy as np
import pytest

import diagnostics_ref as D
import oracle_lib as O
from gpu_support import (DT, DTYPES, OPERATOR_CASES, OPERATOR_IDS, ROOT, STATE, S, assert_same_bits, check_diag,
                         check_reduce, make)

pytestmark = pytest.mark.gpu


def random_state(N, dtype, seed):
    rng = np.random.RandomState(seed)
    f = {n: (0.05 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in ("u", "v", "w")}
    f["dens"] = (0.5 + 0.2 * rng.standard_normal((N + 2,) * 3)).astype(dtype)
    return f


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,P,transport", OPERATOR_CASES, ids=OPERATOR_IDS)
def test_every_op_and_the_struct_match_the_reference(N, P, transport, dtype):
    rng = np.random.RandomState(300 + N + P)
    x = (rng.standard_normal((N + 2,) * 3) * 10.0 ** rng.randint(-2, 3, (N + 2,) * 3)).astype(dtype)
    f = random_state(N, dtype, 400 + N + P)
    with make(N, dtype, P=P, transport=transport) as fs:
        g0 = fs.transport_info()["rccl_groups"]
        fs.upload("user1", x)
        for n in STATE:
            fs.upload(n, f[n])
        check_reduce(fs, "user1", x, f"N={N} P={P} {transport}")
        check_reduce(fs, "user2", np.zeros_like(x), "unallocated slot")  # allocated on first use: zeros
        check_diag(fs, f, f"N={N} P={P} {transport}")
        assert_same_bits(fs.download("user1"), x, "user1 after the calls")
        for n in STATE:
            assert_same_bits(fs.download(n), f[n], f"{n} after the calls")
        if transport == "rccl-self":  # one collective per call went through the communicator
            assert fs.transport_info()["rccl_groups"] - g0 == 2 * len(D.OPS) + 1
        else:
            assert fs.transport_info()["rccl_groups"] == g0
        for bad in ((-1, 0), (6, 0), (0, -1), (0, 12)):
            with pytest.raises(S().SfError) as e:
                fs.reduce(*bad)
            assert e.value.status == S().SF_ERR_INVALID
        assert S().lib.sf_reduce(fs._h, 0, 0, None) == S().SF_ERR_INVALID
        assert S().lib.sf_diagnostics_get(fs._h, None) == S().SF_ERR_INVALID


@pytest.mark.parametrize("P", [1, 4])
def test_bench_size(P):
    N, dtype = 256, np.float32
    f = random_state(N, dtype, 9)
    with make(N, dtype, P=P) as fs:
        for n in STATE:
            fs.upload(n, f[n])
        check_diag(fs, f, f"256^3 P={P}")
        check_reduce(fs, "dens", f["dens"], f"256^3 P={P}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,P,K", [(40, 1, 6), (40, 4, 6), (64, 2, 7), (17, 1, 3)])
def test_max_div_is_the_div_of_project(N, P, K, dtype):
    """diagnostics().max_div of a velocity is reduce(MAX_ABS) of the div slot sf_project then computes from it (SPEC §3:
    lin_solve only reads x0 = div, so div survives the solve);
    the projected state is compared with the reference as well."""
    f = random_state(N, dtype, 50 + N)
    for b, n in ((1, "u"), (2, "v"), (3, "w")):
        O.set_bnd(b, f[n])
    with make(N, dtype, K=K, P=P) as fs:
        for n in STATE:
            fs.upload(n, f[n])
        before = check_diag(fs, f, "before project")
        fs.project("u", "v", "w", "u0", "v0")
        fs.sync()
        div = fs.download("v0")
        got = fs.reduce("max_abs", "v0")
        assert D.bits(got) == D.bits(D.reduce("max_abs", div))
        # the reference's own div of the uploaded velocity, and the slot sf_project left: all the same bits
        assert D.bits(before["max_div"]) == D.bits(got)
        after = {n: fs.download(n) for n in STATE}
        check_diag(fs, after, "after project")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,P", [(40, 4), (34, 2)])
def test_injected_nan_and_inf(N, P, dtype):
    """Single NaN / inf cells on the first and the last plane of a slab and in the last (ragged, for N = 34) vector of a
    row: exact counts, extrema of the finite cells, P = 1 equals P slabs."""
    nzl = N // P
    f = random_state(N, dtype, 77)
    x = f["dens"].copy()
    cells = [(nzl + 1, 1, N), (2 * nzl, N, N - 1), (1, 3, 1), (N, N, N), (nzl, 2, N - 2)]
    for n, (k, j, i) in enumerate(cells):
        x[k, j, i] = (np.nan, np.inf, -np.inf)[n % 3]
    f["u"][cells[0]] = np.inf
    f["w"][cells[1]] = np.nan
    f["dens"][cells[3]] = -np.inf
    f["v"][cells[3]] = np.nan  # the same cell as dens: counted once
    results = []
    for slabs in (1, P):
        with make(N, dtype, P=slabs) as fs:
            fs.upload("user0", x)
            for n in STATE:
                fs.upload(n, f[n])
            check_reduce(fs, "user0", x, f"P={slabs}")
            assert fs.reduce("count_nonfinite", "user0") == len(cells)
            d = check_diag(fs, f, f"P={slabs}")
            assert d["nonfinite"] == 3
            results.append({k: D.bits(v) for k, v in d.items()})
    assert results[0] == results[1]
    clean = random_state(N, dtype, 77)
    ref = D.diagnostics(clean["u"], clean["v"], clean["w"], clean["dens"], DT)
    for name in ("cfl_y", "dens_max"):  # maxima whose field kept all its finite cells' extrema
        assert results[0][name] == D.bits(ref[name])


@pytest.mark.parametrize("P,transport", [(1, "copy"), (4, "copy"), (2, "rccl-self")])
def test_calls_do_not_change_a_later_step(P, transport):
    N, dtype, steps = 32, np.float32, 2
    rng = np.random.RandomState(21)
    f = {n: (0.1 * rng.standard_normal((N + 2,) * 3)).astype(dtype) for n in S().FIELD_NAMES}
    for n in ("u", "v", "w"):
        f[n] = (0.05 * rng.standard_normal((N + 2,) * 3)).astype(dtype)
    out = []
    for watch in (False, True):
        with make(N, dtype, P=P, transport=transport) as fs:
            for n, a in f.items():
                fs.upload(n, a)
            for _ in range(steps):
                if watch:
                    fs.diagnostics()
                fs.vel_step()
                if watch:
                    fs.reduce("sum_sq", "u")
                    fs.diagnostics()
                fs.dens_step()
                if watch:
                    fs.reduce("max_abs", "v0")
            fs.sync()
            out.append({n: fs.download(n) for n in S().FIELD_NAMES})
    for n in S().FIELD_NAMES:
        assert_same_bits(out[1][n], out[0][n], f"{n} with and without diagnostics calls")


def read_frame(path, N):
    """density and velocity (interior cells, float32) of a binary frame of sf_driver."""
    raw = open(path, "rb").read()

    def block(tag, count):
        at = raw.index(tag) + len(tag)
        return np.frombuffer(raw, ">f4", count, at).astype(np.float32)

    dens = block(b"LOOKUP_TABLE default\n", N ** 3).reshape(N, N, N)
    vel = block(b"VECTORS velocity float\n", 3 * N ** 3).reshape(N, N, N, 3)
    return dens, vel


def test_driver_monitor_lines(tmp_path):
    """sf_driver --n 64 --steps 20 --monitor 5: four lines whose numbers equal the reference on the states the same run
    wrote as frames (the interior cells; the shells of u, v, w are those of set_bnd, which vel_step leaves)."""
    N = 64
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    run = subprocess.run([exe, "--n", str(N), "--steps", "20", "--monitor", "5", "--every", "5", "--binary", "--quiet",
                          "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("monitor ")]
    print("\n".join(lines))
    assert len(lines) == 4
    for frame, ln in enumerate(lines):
        m = re.fullmatch(r"monitor step=(\d+) mass=(\S+) kinetic=(\S+) max_div=(\S+) cfl=(\S+) nonfinite=(\d+)", ln)
        assert m, ln
        assert int(m.group(1)) == 5 * frame
        dens, vel = read_frame(tmp_path / f"anim_s{frame}.vtk", N)
        f = {}
        for b, n in ((1, "u"), (2, "v"), (3, "w")):
            f[n] = np.zeros((N + 2,) * 3, np.float32)
            f[n][1:-1, 1:-1, 1:-1] = vel[..., b - 1]
            O.set_bnd(b, f[n])
        f["dens"] = np.zeros((N + 2,) * 3, np.float32)
        f["dens"][1:-1, 1:-1, 1:-1] = dens
        want = D.diagnostics(f["u"], f["v"], f["w"], f["dens"], DT)
        for q, name in enumerate(("mass", "kinetic", "max_div", "cfl"), 2):
            assert D.bits(float(m.group(q))) == D.bits(want[name]), (ln, name, want[name])
        assert int(m.group(6)) == want["nonfinite"] == 0


def test_driver_stops_on_a_nonfinite_state():
    """--buoyancy 1e39 is finite as a double and +inf as the fp32 coefficient: the force is +-inf or NaN in every cell,
    so the velocity is not finite after the first step. The driver names the step and exits with status 3."""
    exe = os.path.join(ROOT, "fluidsolvergpu_amd", "sf_driver")
    run = subprocess.run([exe, "--n", "16", "--steps", "6", "--monitor", "2", "--every", "0", "--quiet",
                          "--buoyancy", "1e39"], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr)
    assert run.returncode == 3
    assert "not finite after step 0" in run.stderr
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("monitor ")]
    assert len(lines) == 1 and int(lines[0].rsplit("nonfinite=", 1)[1]) > 0
