"""The shared comparison and the context factory of tests/gpu_support.py hold what the GPU suites rely on (no GPU
needed): assert_same_bits sees a signed zero, one ulp and a NaN payload; make passes exactly the keyword arguments the
suites passed before they shared it; traced_plans reads the pass plan of a preconditioned solve out of a schedule trace."""
import numpy as np
import pytest

import gpu_support as G


def field(dtype, value=1.5):
    return np.full((3, 4, 5), value, dtype)


def with_cell(a, value):
    b = a.copy()
    b[1, 2, 3] = value
    return b


def nan_with_payload(dtype, payload):
    """A quiet NaN whose low mantissa bits hold `payload`."""
    uint, quiet = (np.uint32, 0x7FC00000) if dtype == np.float32 else (np.uint64, 0x7FF8000000000000)
    x = np.array([quiet | payload], uint).view(dtype)[0]
    assert np.isnan(x)
    return x


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
def test_assert_same_bits(dtype):
    a = field(dtype)
    G.assert_same_bits(a, a.copy(), "equal")
    G.assert_same_bits(a, a.copy(), "equal", nan_ok=True)
    nan1, nan2 = nan_with_payload(dtype, 1), nan_with_payload(dtype, 2)
    differ = [("signed zero", with_cell(a, -0.0), with_cell(a, 0.0)),
              ("one ulp", with_cell(a, np.nextafter(dtype(1.5), dtype(2))), a),
              ("NaN payload", with_cell(a, nan1), with_cell(a, nan2)),
              ("NaN against a number", with_cell(a, nan1), a),
              ("a number against NaN", a, with_cell(a, nan1))]
    for what, got, want in differ:
        with pytest.raises(AssertionError, match=r"1 entries differ, first at \[k,j,i\]=\[1 2 3\]"):
            G.assert_same_bits(got, want, what)
    for what, got, want in differ:
        if what == "NaN payload":
            G.assert_same_bits(got, want, what, nan_ok=True)
        else:
            with pytest.raises(AssertionError, match="1 entries differ"):
                G.assert_same_bits(got, want, what, nan_ok=True)
    G.assert_same_bits(with_cell(a, nan1), with_cell(a, nan1), "the same NaN")
    with pytest.raises(AssertionError):
        G.assert_same_bits(a, a.astype(np.float32 if dtype == np.float64 else np.float64), "other precision")
    with pytest.raises(AssertionError):
        G.assert_same_bits(a, a[1:], "other shape")


class Recorder:
    """Stands in for fluidsolvergpu_amd.solver: FluidSolver records its arguments."""

    SF_FLAG_RCCL_SELF = 2

    def __init__(self):
        self.calls = []

    def FluidSolver(self, *args, **kw):
        self.calls.append((args, kw))
        return kw


@pytest.fixture
def recorder(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(G, "S", lambda: r)
    return r


def test_make_passes_the_keyword_arguments_of_every_call_site(recorder):
    base = dict(dtype="f32", iters=4, dt=0.1, diff=1e-4, visc=1e-4)
    assert G.make(24, np.float32) == base
    assert G.make(24, np.float32, P=1, transport="rccl-self") == base
    assert G.make(24, np.float32, P=3, transport="copy") == dict(base, nslabs_local=3)
    assert G.make(24, np.float32, P=3) == dict(base, nslabs_local=3)
    assert G.make(24, np.float32, P=4, transport="rccl-self") == dict(base, nslabs_local=4, flags=recorder.SF_FLAG_RCCL_SELF)
    assert G.make(24, np.float64, K=9, P=2) == dict(base, dtype="f64", iters=9, nslabs_local=2)
    # the parity family: the dictionary of slab_kw goes through as it is
    assert G.slab_kw("rccl-self", 1) == {"nslabs_local": 1} and G.slab_kw("copy", 1) == {"nslabs_local": 1}
    assert G.slab_kw("copy", 8) == {"nslabs_local": 8} and G.slab_kw("rccl-self", 2) == {"nslabs_local": 2, "flags": 2}
    for transport in ("copy", "rccl-self"):
        for P in (1, 2, 8):
            assert G.make(24, np.float32, K=7, **G.slab_kw(transport, P)) == dict(base, iters=7, **G.slab_kw(transport, P))
    assert G.make(16, np.float32, nslabs_local=4) == dict(base, nslabs_local=4)
    assert all(args in ((24,), (16,)) for args, _ in recorder.calls)  # N is the one positional argument
    assert (G.DT, G.DIFF, G.VISC) == (0.1, 1e-4, 1e-4)


def test_the_solver_flag_is_the_literal_of_slab_kw():
    from fluidsolvergpu_amd import solver

    assert solver.SF_FLAG_RCCL_SELF == G.slab_kw("rccl-self", 2)["flags"]
    assert G.NAMES == solver.FIELD_NAMES


# ---- traced_plans on a hand-written trace ---------------------------------------------------------------------------
def op(name, slab, stream, *acc):
    return {"t": "op", "name": name, "slab": slab, "stream": stream, "acc": [list(a) for a in acc]}


def two_slab_trace():
    """A context of two slabs of 36 planes on G = 4 ghost planes (buffers: r 0, z 1, its partner 2 on slab 0; 5, 6, 7 on
    slab 1). First M(r): 4Z 3+4 2 — the boundary launch of the three-sweep pass reaches 8 planes into the slab, the pair
    snaps back to 4. Second M(r): zero_z, then 4C 4+4. Rows that the parser must skip stand in between."""
    ctx = {"t": "ctx", "N": 72, "P": 2, "L": 2, "rank": 0, "G": 4, "nzl": 36, "np": 44, "trap": 5, "hs_is_bs": 0, "inject": 0}
    dot = [op("cg_dot", s, "cs", ("r", 5 * s, 4, 40), ("r", 5 * s + 1, 4, 40)) for s in (0, 1)]
    rows = [ctx, op("jacobi2", 0, "cs", ("w", 9, 3, 41)),  # (a Jacobi solve before the first r.z: no part of any M)
            *dot,
            op("cg_apply_dot", 0, "cs", ("r", 3, 3, 41)),
            op("jacobi4", 0, "bs", ("r", 0, 1, 11), ("w", 2, 3, 8), ("r", 0, 33, 43), ("w", 2, 36, 40)),
            op("jacobi4", 1, "bs", ("r", 5, 1, 11), ("w", 7, 4, 8), ("r", 5, 33, 43), ("w", 7, 36, 41)),
            op("jacobi4", 0, "cs", ("r", 0, 5, 39), ("w", 2, 8, 36)),
            {"t": "xchg", "seq": 7, "G": 4, "fields": [12]},
            op("halo", 0, "hs", ("r", 7, 4, 8), ("w", 2, 40, 44)),
            {"t": "rec", "slab": 0, "stream": "bs", "ev": "boundary"},
            op("jacobi3", 0, "bs", ("r", 2, 0, 15), ("r", 0, 1, 14), ("w", 1, 3, 12), ("r", 2, 29, 43), ("w", 1, 32, 40)),
            op("jacobi3", 0, "cs", ("r", 2, 9, 35), ("w", 1, 12, 32)),
            op("jacobi2", 0, "bs", ("r", 1, 2, 10), ("w", 2, 3, 8), ("w", 2, 36, 40)),
            op("jacobi2", 0, "cs", ("r", 1, 6, 38), ("w", 2, 8, 36)),
            *dot,
            op("zero_z", 0, "cs", ("w", 2, 0, 44)),
            op("jacobi4", 0, "bs", ("r", 2, 0, 12), ("w", 1, 3, 8), ("w", 1, 36, 40)),
            op("jacobi4", 0, "cs", ("r", 2, 4, 40), ("w", 1, 8, 36)),
            op("jacobi4", 0, "bs", ("r", 1, 0, 16), ("w", 2, 3, 12), ("w", 2, 32, 40)),
            op("jacobi4", 0, "cs", ("r", 1, 8, 36), ("w", 2, 12, 32)),
            *dot,
            op("jacobi1", 0, "cs", ("w", 1, 3, 41))]  # (after the last r.z: an unfinished window is no plan)
    return rows


def test_traced_plans(tmp_path):
    import json

    path = tmp_path / "trace.jsonl"
    one_slab = [{"t": "ctx", "N": 40, "P": 1, "G": 1, "trap": 5},
                op("cg_dot", 0, "cs"), op("zero_z", 0, "cs", ("w", 1, 0, 42)), op("jacobi1", 0, "cs", ("w", 2, 0, 42)),
                op("cg_dot", 0, "cs"),
                # two passes of one name: told apart by the buffer they write; pairs on G = 1 are two planes deep
                op("jacobi2", 0, "cs", ("w", 2, 0, 42)), op("jacobi2", 0, "cs", ("w", 1, 0, 42)),
                op("jacobi3", 0, "cs", ("w", 2, 0, 42)), op("jacobi1", 0, "cs", ("w", 1, 0, 42)),
                op("cg_dot", 0, "cs")]
    path.write_text("".join(json.dumps(r) + "\n" for r in two_slab_trace() + one_slab))
    (ctx2, plans2), (ctx1, plans1) = G.traced_plans(str(path))
    assert (ctx2["G"], ctx2["P"], ctx2["trap"]) == (4, 2, 5) and plans2 == ["4Z 3+4 2", "4C 4+4"]
    assert ctx1["P"] == 1 and plans1 == ["1C", "2Z 2 3 1"]


def test_passes_of_M_on_a_live_trace(tmp_path):
    """slab0_ops leaves out other slabs, other records and a line still being written; passes_of_M counts the passes
    that write the two buffers cg_dot reads z from, and no pass of another solve."""
    import json

    rows = [{"t": "ctx", "N": 40, "P": 1, "G": 1, "trap": 5},
            op("jacobi2", 0, "cs", ("r", 3, 0, 42), ("w", 9, 0, 42)),   # diffuse: its buffers are not z's
            op("jacobi2", 0, "cs", ("w", 1, 0, 42)), op("cg_dot", 0, "cs", ("r", 0, 1, 41), ("r", 1, 1, 41), ("w", 7, 0, 42)),
            {"t": "rec", "slab": 0, "stream": "cs", "ev": "cs_mark"}, op("jacobi1", 1, "cs", ("w", 2, 0, 42)),
            op("jacobi2", 0, "cs", ("w", 2, 0, 42)), op("cg_dot", 0, "cs", ("r", 0, 1, 41), ("r", 2, 1, 41), ("w", 7, 0, 42)),
            op("jacobi2", 0, "cs", ("w", 1, 0, 42)), op("cg_dot", 0, "cs", ("r", 0, 1, 41), ("r", 1, 1, 41), ("w", 7, 0, 42))]
    path = tmp_path / "trace.jsonl"
    path.write_text("".join(json.dumps(r) + "\n" for r in rows) + '{"t":"op","name":"jaco')
    ops = G.slab0_ops(str(path))
    assert len(ops) == 7
    assert G.passes_of_M(ops) == (3, {1, 2}, 1)
    assert G.passes_of_M(ops[:3]) == (1, {1}, 1)
