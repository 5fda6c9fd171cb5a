"""The lifetime of a context: four times over, a context is created, made to allocate everything it allocates lazily
(user slots, snapshot buffers and their stream and event, tracer buffers of three sizes, reduction records, the CG state,
the preconditioner's fields, the multigrid levels, the copy-bandwidth buffers of two sizes) and closed. A later context
must compute exactly what the first one did, and the device must have its memory back after every close().

N = 64 is the smallest size at which every one of these resources exists: a four-level hierarchy, 16 planes per slab at
P = 4 and ghost depth 2. No case provokes a failing allocation; the failure paths are tests/own_check.cpp's.

Free device memory is read with hipMemGetInfo of the HIP runtime libsfgpu.so runs on, after close() and a
hipDeviceSynchronize: the call torch.cuda.mem_get_info() makes, without a second runtime in the process (torch brings
its own, and the library is loaded first here). The readings of this build and of the parent build, per case and cycle,
are in profiles/r18_context_lifetime.txt."""
import ctypes

import numpy as np
import pytest

from gpu_support import DTYPE_IDS, DTYPES, STATE, assert_same_bits, check_transport, make, random_fields, upload_all

pytestmark = pytest.mark.gpu

N, K, CYCLES = 64, 4, 4
CONTEXTS = [(1, "copy"), (2, "copy"), (4, "rccl-self")]  # the last two: mg_cases.DECOMPOSED at max_levels = 0


def free_bytes():
    with open("/proc/self/maps") as maps:  # the runtime that is loaded already, by libsfgpu.so
        hip = ctypes.CDLL(next(line.split()[-1] for line in maps if "libamdhip64" in line))
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def tracer_positions(n, dtype):
    rng = np.random.RandomState(100 + n)
    return rng.uniform(-1.0, N + 2.0, size=(n, 3)).astype(dtype)


def cycle(dtype, P, transport):
    """One context from create to close(): (everything it returned, in order, as (name, array); bytes_per_field)."""
    out = []

    def keep(what, value):
        if isinstance(value, dict):
            for k in sorted(value):
                keep(f"{what}.{k}", value[k])
        elif isinstance(value, (tuple, list)):
            for q, v in enumerate(value):
                keep(f"{what}[{q}]", v)
        else:
            a = np.atleast_1d(value)
            out.append((what, a.astype(np.float64) if a.dtype.kind in "iub" else a.copy()))

    def fields(what, names):
        for n in names:
            keep(f"{what}: {n}", fs.download(n))

    with make(N, dtype, K=K, P=P, transport=transport) as fs:
        nbytes = fs.layout_info()["bytes_per_field"]
        upload_all(fs, random_fields(N, dtype, 18))                                    # 1
        for q in range(4):                                                             # 2
            fs.fill(f"user{q}", 0.01 * (q + 1))
        fs.bind_sources()
        fs.vel_step()                                                                  # 3
        fs.dens_step()
        fields("step", STATE)
        fs.snapshot(list(STATE))                                                       # 4
        keep("snapshot 3", fs.snapshot_read(3))
        fs.tracers_set(tracer_positions(1000, dtype))                                  # 5
        fs.tracers_set(tracer_positions(300, dtype))
        fs.tracers_set_capacity(16)
        fs.tracers_advect()
        keep("tracers", fs.tracers_get_owned())
        keep("sum of dens", fs.reduce("sum", "dens"))                                  # 6
        keep("diagnostics", fs.diagnostics())
        fs.set_pressure_sync(4)                                                        # 7
        fs.set_pressure_preconditioner("jacobi", 3)
        keep("jacobi solve", fs.project_cg("u", "v", "w", "u0", "v0", 1e-3, 3))
        fields("jacobi solve", ("u", "v", "w", "u0", "v0"))
        fs.set_pressure_multigrid(2, 0, 8)                                             # 8
        fs.precondition("user0", "user1")
        fields("precondition", ("user0",))
        keep("multigrid solve", fs.project_cg("u", "v", "w", "u0", "v0", 1e-3, 2))
        fields("multigrid solve", ("u", "v", "w", "u0", "v0"))
        for nb in (1 << 20, 2 << 20):                                                  # 9
            assert fs.copy_bandwidth_gbps(nb, 1) > 0
        check_transport(fs, transport, P)
    return out, nbytes


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("P,transport", CONTEXTS, ids=[f"P{p}-{t}" for p, t in CONTEXTS])
def test_contexts_come_and_go(P, transport, dtype):
    first, free = None, []
    for c in range(1, CYCLES + 1):
        got, nbytes = cycle(dtype, P, transport)
        free.append(free_bytes())
        print(f"P={P} {transport} {np.dtype(dtype).name}: free after cycle {c}: {free[-1]} bytes "
              f"(bytes_per_field {nbytes})")
        if first is None:
            first = got
            continue
        # a context must not see what an earlier one left behind
        assert [w for w, _ in got] == [w for w, _ in first]
        for (what, a), (_, want) in zip(got, first):
            assert_same_bits(a, want, f"cycle {c}: {what}")
    # A context of these cases holds more than twenty buffers of bytes_per_field per slab: a context leaked per cycle
    # would lose more than thirty times this bound over the three cycles, a single leaked field per cycle 1.5 times.
    lost = free[0] - free[-1]
    print(f"P={P} {transport} {np.dtype(dtype).name}: lost between cycle 1 and cycle {CYCLES}: {lost} bytes, "
          f"bound {2 * nbytes}")
    assert lost <= 2 * nbytes, (free, nbytes)
