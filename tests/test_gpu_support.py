"""The shared comparison and the context factory of tests/gpu_support.py hold what the GPU suites rely on (no GPU
needed): assert_same_bits sees a signed zero, one ulp and a NaN payload; make passes exactly the keyword arguments the
suites passed before they shared it."""
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
