"""CPU side of the decomposed-tracer ABI (docs/SPEC.md §6.1): the new status and entry points, no GPU needed."""


def test_tracer_overflow_status():
    from fluidsolvergpu_amd import solver

    assert solver.SF_ERR_TRACER_OVERFLOW == 6
    assert solver.lib.sf_status_string(6) == b"SF_ERR_TRACER_OVERFLOW"
    assert solver.lib.sf_status_string(7) == b"SF_ERR_UNKNOWN"


def test_tracer_entry_points_reject_a_null_context():
    import ctypes as C

    from fluidsolvergpu_amd import solver

    n = C.c_int(-1)
    assert solver.lib.sf_tracers_owned(None, C.byref(n)) == solver.SF_ERR_INVALID
    assert solver.lib.sf_tracers_get_owned(None, None, None, None, None) == solver.SF_ERR_INVALID
    assert solver.lib.sf_tracers_set_capacity(None, 10) == solver.SF_ERR_INVALID
