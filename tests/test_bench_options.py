"""bench.py's options on CPU: a plain run reports the timed steps only, `--full` adds the other legs, and
`--dump-outputs DIR` writes what the timed path computed. The runs use the solver stand-in of SF_BENCH_DRYRUN=1
(tests/bench_dryrun_stub.py); dump_outputs itself is checked against a field whose every value is known."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from gpu_support import ROOT, free_port

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype")
FULL_ONLY = ("step_times_ms", "hbm_copy_gbps_same_run", "single_gpu", "speedup", "roofline", "roofline_cache_resident",
             "cpu_baseline", "parity_in_run")


class _KnownField:
    """Stands in for a solver context: cell c of field q holds (q + 1) * c, c the flat index into the (N+2)^3 array."""

    def __init__(self, N, np_dtype):
        self.N, self.np_dtype = N, np_dtype

    def download_planes(self, field, kb, ke):
        S = self.N + 2
        q = bench.DUMP_FIELDS.index(field)
        return ((q + 1) * np.arange(kb * S * S, ke * S * S, dtype=np.float64)).astype(self.np_dtype).reshape(-1, S, S)


@pytest.mark.parametrize("N,np_dtype", [(14, np.float32), (256, np.float32), (256, np.float64)])
def test_dump_outputs_values(N, np_dtype, tmp_path):
    S = N + 2
    info = bench.dump_outputs(_KnownField(N, np_dtype), N, None, str(tmp_path))
    whole = info["whole"]
    assert whole == (N == 14)
    idx = np.arange(S ** 3, dtype=np.float64) if whole else np.load(tmp_path / "sample_index.npy")
    if not whole:
        assert idx.dtype == np.float64 and idx.shape == (bench.DUMP_SAMPLE,)
        assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < S ** 3
        want_idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(S ** 3, bench.DUMP_SAMPLE, replace=False))
        assert np.array_equal(idx, want_idx.astype(np.float64))
    total = 0
    for q, name in enumerate(bench.DUMP_FIELDS):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np_dtype and a.shape == ((S, S, S) if whole else (bench.DUMP_SAMPLE,))
        assert np.array_equal(a.ravel(), ((q + 1) * idx).astype(np_dtype))
        total += a.nbytes
    if not whole:
        total += idx.nbytes
    assert total <= bench.DUMP_BYTES
    assert info["cells_per_field"] == (S ** 3 if whole else bench.DUMP_SAMPLE)


def _run_bench(world, args, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(OMP_NUM_THREADS="1", SF_BENCH_DRYRUN="1")
    script = os.path.join(ROOT, "bench.py")
    if world == 1:
        cmd = [sys.executable, script]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), script]
    r = subprocess.run(cmd + ["--gpus", str(world)] + args, capture_output=True, text=True, timeout=300, env=env,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("world,N", [(1, 16), (2, 16), (2, 256)])
def test_plain_run_with_dump(world, N, tmp_path):
    """No --full: the contract fields and nothing that needs a run of its own; the dump holds every field (whole at
    16^3, the seeded sample at 256^3, gathered over the ranks in global order)."""
    out = tmp_path / "dump"
    d = _run_bench(world, ["--steps", "3", "--warmup", "1", "--grid", str(N), "--dump-outputs", str(out)], tmp_path)
    for key in CONTRACT:
        assert key in d, key
    for key in FULL_ONLY:
        assert key not in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == world and d["data"].startswith("DRYRUN")
    S = N + 2
    whole = d["outputs_dumped"]["whole"]
    assert whole == (N == 16)
    for name in bench.DUMP_FIELDS:
        a = np.load(out / f"{name}.npy")
        assert a.shape == ((S, S, S) if whole else (bench.DUMP_SAMPLE,)) and a.dtype == np.float32
        assert (a == 1.0).all()  # the stand-in's download_planes: ones everywhere
    assert (out / "sample_index.npy").exists() == (not whole)


def test_full_run_single_gpu(tmp_path):
    """--full at N = 1 keeps the legs a plain run leaves out."""
    d = _run_bench(1, ["--steps", "2", "--warmup", "1", "--grid", "8", "--roofline-n", "8", "--cpu-steps", "1",
                       "--full"], tmp_path)
    for key in CONTRACT + ("step_times_ms", "hbm_copy_gbps_same_run", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["step_times_ms"]["n"] == 2 and "outputs_dumped" not in d
