"""The batched protocol of docs/SPEC.md §11 "Where the scalars are computed" on the CPU (no GPU, no library): the numpy
model of tests/pressure_cg_device_model.py, layered on tests/pressure_cg_ref.py,

(a) returns the reference's bits — fields, status, iterations, rel_residual — for every check_every on the inputs of
    tests/test_pressure_cg_device_gpu.py, with the host waits the SPEC states;
(b) run as three wrong protocols (the mutants of the model), differs from the reference on the input named in the test
    id, which is the GPU case that would catch that error in the library, and equals it on an input that cannot."""
import numpy as np
import pytest

import diagnostics_ref as D
import pressure_cg_device_model as M
import pressure_cg_ref as R
import shape_cases as C
from ref_support import same_bits

TOL = 1e-3
MS = (1, 3, 5, 8)


def same_outcome(a, b):
    return ((a["status"], a["iterations"]) == (b["status"], b["iterations"])
            and D.bits(a["rel_residual"]) == D.bits(b["rel_residual"])
            and all(same_bits(a[n], b[n]) for n in ("u", "v", "w", "p", "div")))


def inputs():
    """name -> (u, v, w, tol, max_iters): small random solves and the stop cases of the GPU file."""
    out = {}
    for N, dtype in ((1, np.float32), (2, np.float64), (3, np.float32), (5, np.float64), (13, np.float32), (34, np.float32)):
        out[f"random-N{N}-{C.dname(dtype)}"] = (*C.cg_velocity(N, dtype, C.cg_seed(N)), TOL, 8)
    out.update(M.stop_inputs())
    return out


INPUTS = inputs()
_REFERENCES = {}


def reference(name):
    if name not in _REFERENCES:
        u, v, w, tol, max_iters = INPUTS[name]
        _REFERENCES[name] = R.project_cg(u, v, w, tol, max_iters)
    return _REFERENCES[name]


@pytest.mark.parametrize("name", list(INPUTS))
def test_the_result_does_not_depend_on_check_every(name):
    u, v, w, tol, max_iters = INPUTS[name]
    want = reference(name)
    for m in MS + (max(max_iters, 1),):
        got = M.project_cg_batched(u, v, w, tol, max_iters, m)
        assert same_outcome(got, want), (name, m, got["status"], got["iterations"], want["status"], want["iterations"])
        assert 1 <= got["host_waits"] <= -(-want["iterations"] // m) + 1
        if m >= max_iters:
            assert got["host_waits"] == 1


def test_the_inputs_stop_where_their_names_say():
    for t in ("f32", "f64"):
        assert (reference(f"zero-{t}")["status"], reference(f"zero-{t}")["iterations"]) == (R.CONVERGED, 0)
        assert (reference(f"nan-{t}")["status"], reference(f"nan-{t}")["iterations"]) == (R.BREAKDOWN, 0)
        assert reference(f"+inf-{t}")["status"] == reference(f"-inf-{t}")["status"] == R.BREAKDOWN
        assert (reference(f"max_iters0-{t}")["status"], reference(f"max_iters0-{t}")["iterations"]) == (R.MAX_ITERS, 0)
        assert (reference(f"max_iters1-{t}")["status"], reference(f"max_iters1-{t}")["iterations"]) == (R.MAX_ITERS, 1)
        assert (reference(f"tol1e30-{t}")["status"], reference(f"tol1e30-{t}")["iterations"]) == (R.CONVERGED, 1)
        assert (reference(f"tol1e-200-{t}")["status"], reference(f"tol1e-200-{t}")["iterations"]) == (R.MAX_ITERS, 12)
        assert (reference(f"stop_at_2-{t}")["status"], reference(f"stop_at_2-{t}")["iterations"]) == (R.CONVERGED, 2)
    for N, dtype, _, iterations in M.DELTA_BREAKDOWN:
        ref = reference(f"delta-N{N}-{C.dname(dtype)}")
        assert (ref["status"], ref["iterations"]) == (R.BREAKDOWN, iterations)
        assert np.isfinite(ref["rel_residual"]) and np.isfinite(ref["p"]).all()  # delta, not rho', broke down


# (mutant, the input that tells it from the reference at m = 5, an input that cannot, the GPU case that runs the first)
MUTANT_CASES = [
    ("no_freeze", "stop_at_2-f32", "max_iters1-f32", "test_stop_cases[stop_at_2-f32-m5]"),
    ("no_freeze", "stop_at_2-f64", "tol1e-200-f64", "test_stop_cases[stop_at_2-f64-m5]"),
    ("no_freeze", "tol1e30-f32", "max_iters0-f32", "test_stop_cases[tol1e30-f32-m5]"),
    ("count_enqueued", "stop_at_2-f32", "tol1e-200-f32", "test_stop_cases[stop_at_2-f32-m5]"),
    ("count_enqueued", "zero-f64", "max_iters0-f64", "test_stop_cases[zero-f64-m5]"),
    ("count_enqueued", "nan-f32", "max_iters1-f32", "test_stop_cases[nan-f32-m5]"),
    ("late_freeze", "delta-N4-f32", "stop_at_2-f32", "test_stop_cases[delta-N4-f32-m5]"),
    ("late_freeze", "delta-N3-f64", "nan-f64", "test_stop_cases[delta-N3-f64-m5]"),
    ("late_freeze", "delta-N2-f32", "zero-f32", "test_stop_cases[delta-N2-f32-m1]"),
]


@pytest.mark.parametrize("mut,caught_on,blind_on,gpu_case", MUTANT_CASES,
                         ids=[f"{m}-caught-by-{g}" for m, _, _, g in MUTANT_CASES])
def test_the_inputs_tell_the_wrong_protocols(mut, caught_on, blind_on, gpu_case):
    m = int(gpu_case.rsplit("-m", 1)[1].rstrip("]"))
    u, v, w, tol, max_iters = INPUTS[caught_on]
    assert same_outcome(M.project_cg_batched(u, v, w, tol, max_iters, m), reference(caught_on))
    bad = M.project_cg_batched(u, v, w, tol, max_iters, m, mut)
    assert not same_outcome(bad, reference(caught_on)), f"{mut} is the reference on {caught_on}"
    print(f"{mut} on {caught_on}: status {bad['status']} iterations {bad['iterations']}, reference "
          f"{reference(caught_on)['status']} {reference(caught_on)['iterations']}")
    u, v, w, tol, max_iters = INPUTS[blind_on]
    assert same_outcome(M.project_cg_batched(u, v, w, tol, max_iters, m, mut), reference(blind_on)), blind_on
