"""The inputs and the conditions that the tests of docs/SPEC.md §18 (MacCormack under the mask) share:
test_obstacle_maccormack_ref.py on the CPU and test_obstacle_maccormack_gpu.py on the device draw the masks of
tests/obstacle_cases.py and the fields and velocities of tests/obstacle_transport_cases.py (the `specials` inputs: those
of tests/obstacle_special_cases.py), so a case named on one side is the case of the other. References are computed once
and only read afterwards."""
import numpy as np

import obstacle_cases as OC
import obstacle_maccormack_ref as MM
import obstacle_special_cases as SP
import obstacle_transport_cases as TC
import obstacles_ref as OB
from shape_cases import DT, DTYPES, dname

FAMILIES = TC.FAMILIES
SIZES = [1, 2, 3, 5, 13, 34, 65, 70]  # 65, 70: the lane-64 seam and ragged tails of the flat mapping
BS = TC.BS
OPERATORS = [(f, N, t) for f in FAMILIES for N in SIZES for t in DTYPES]
SPECIALS = [(N, t) for N in (5, 13, 34, 65) for t in DTYPES]  # the `specials` inputs under `box`
DECOMPOSED = [(f, N, P, tr) for N, P in ((34, 2), (34, 17), (64, 4), (40, 2)) for f in ("box", "random30")
              for tr in ("copy", "rccl-self")]
MC, SL = MM.MACCORMACK, MM.SEMI_LAGRANGIAN
SCHEMES = ((MC, MC), (MC, SL), (SL, MC))
_CACHE = {}


def once(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def decomposed_dtype(P):
    return np.float32 if P != 17 else np.float64


def inputs(family, N, dtype, b, one_plane=False):
    """(d0, (u, v, w)) of an ordinary case."""
    return TC.fields(family, N, dtype, b)[1], TC.velocity(family, N, dtype, one_plane)


def special_inputs(N, dtype, b):
    """(d0, (u, v, w)) of the `specials` family under `box`."""
    d0, u, v, w, _ = SP.advect_inputs("specials", "box", OC.mask("box", N, dtype), b)
    return d0, (u, v, w)


def run(mask, d0, vel, b, wrong=None, slabs=1):
    d = np.zeros_like(d0)
    return MM.advect_mc_masked(b, d, d0, *vel, DT, mask, wrong, slabs)


def want(family, N, dtype, b, one_plane=False, P=None):
    """The reference's result of an ordinary case (P: the slab count the mask is drawn for; the reference is P = 1)."""
    def build():
        d0, vel = inputs(family, N, dtype, b, one_plane)
        return run(OC.mask(family, N, dtype, P), d0, vel, b)
    return once(("advect", family, N, dname(dtype), b, one_plane, P), build)


def want_special(N, dtype, b):
    def build():
        d0, vel = special_inputs(N, dtype, b)
        return run(OC.mask("box", N, dtype), d0, vel, b)
    return once(("specials", N, dname(dtype), b), build)


def far_reverse_velocity(family, N, dtype):
    """TC.velocity for two slabs with one cell, on the last plane of the first slab, whose w = +6.5 / dt0: its forward
    trace stays inside its own slab (6.5 planes towards the wall side) and only the reverse trace crosses 6.5 planes into
    the second slab, more than the ghost planes a slab stores (four at most)."""
    u, v, w = TC.velocity(family, N, dtype, one_plane=True)
    w[N // 2, N // 2, N // 2] = 6.5 / (DT * N)
    return u, v, w


# ---- the conditions ------------------------------------------------------------------------------------------------
def second_order_share(family, N, dtype, b=0, one_plane=False, P=None):
    """Counts of MM.outcomes for the case, on the reference."""
    d0, vel = inputs(family, N, dtype, b, one_plane)
    return MM.outcomes(MM.parts(b, d0, *vel, DT, OC.mask(family, N, dtype, P)))


def check_second_order(family, N, dtype, one_plane=False, P=None):
    """At least a quarter of the fluid cells of a `box` case from N = 13 up take the corrected value, so a comparison
    of such a case compares the second-order branch and not the fallback alone. Returns the counts."""
    o = second_order_share(family, N, dtype, 0, one_plane, P)
    if family == "box" and N >= 13:
        assert 4 * o["second"] >= o["fluid"], (family, N, o)
    return o


def check_nan_share(fields, mask, what):
    """Fewer than a quarter of the fluid cells of every compared field of the reference are NaN."""
    return SP.check_nan_share(fields, mask, what)


def fluid_cells(mask):
    return OB.Mask(mask).fluid
