"""The sizes, frames, seeds, inputs and conditions of the tests of orthographic volume rendering (docs/SPEC.md §13),
shared by tests/test_render_view_ref.py (CPU: the conditions hold, every wrong variant of the reference is told from it
on a named case) and tests/test_render_view_gpu.py (GPU: every case against the reference in bits).

Inputs: the families of render_cases (random, shells, special, closed), with set_bnd(0, .) applied to the `random` family so
that a sample at a cell centre of the outermost interior layer, which reads the shell with weight zero, equals the cell
(the axis identity of §13.1). In the special family the emission takes NaN and the infinities from N = 13 up only: one
such sample makes its whole ray's C a NaN, and below that size more than a quarter of the pixels are hit (22 of 40 at
N = 5). The density keeps them all: a NaN density is transparent. The closed family is render_cases.closed (zero,
half, opaque) as it stands, at every size and dtype: through the six axis frames, where §12.1 gives the images exactly
(zero: (+0, 1); half: Tr = 2^-N and C = 1 - 2^-N while N fits the mantissa; opaque: Tr = +0 and C = e of the first
cell), and through one oblique frame each (CLOSED_VIEW), where zero is (+0, 1) everywhere and the other two are
compared with the reference. Their shells are zero, which is all the axis identity needs of a shell: finite values.

Sizes: those of the §12 tests up to 130. Directions (from view_frame): (1,2,3); (-2,1,-1), whose chain runs from the
high side; (1,1,0), whose rays stay inside a slab (step_z = 0); (3,-1,2). Steps 0.5, 1 and 1.7 (samples skip planes).
edge_frame puts samples exactly on two faces of the box. Images are chosen for the seams of the 8 x 8 pixel tile, not for N: 1 x 1, 7 x 5, 8 x 8, 9 x 17, 64 x 1, 65 x 3, and
(N+3) x N. The table CASES crosses sizes, dtypes, families and directions, and walks through the steps and images so
that every step meets every image; every size also takes the (N+3) x N image at step 0.5 in every direction, on which
the conditions are stated. Emission alternates; direction (1,2,3) of that image takes both forms.

Conditions (check_conditions; caps reasoned in the issue that introduced §13, not measurements), on the (N+3) x N image
at step 0.5: from N = 13 up (N = 5: `random` only) at least half of the pixels whose ray visits a sample end with
0 < Tr < 1; from N = 5 up at least one ray ends at Tr = 0; in the special family fewer than a quarter of the pixels of
either image are NaN. On every view_frame image of more than one pixel at least one pixel misses the box and is
exactly (+0, 1)."""
import functools
from collections import namedtuple

import numpy as np

import render_cases as RC
import render_ref as RR
import render_view_ref as VR
import shape_cases as SC
import stable_ref as S3
from shape_cases import DTYPES, dname  # noqa: F401

SIZES = [1, 2, 3, 5, 13, 31, 34, 64, 65, 70, 130]
DECOMPOSED = [c for c in SC.DECOMPOSED if c[0] <= 130]
DIRECTIONS = [((1, 2, 3), (0, 0, 1)), ((-2, 1, -1), (0, 1, 0)), ((1, 1, 0), (0, 0, 1)), ((3, -1, 2), (0, 0, 1))]
DIR_IDS = ["d123", "d-21-1", "d110", "d3-12"]
STEPS = [0.5, 1.0, 1.7]
FIXED_IMAGES = [(1, 1), (7, 5), (8, 8), (9, 17), (64, 1), (65, 3)]
FAMILIES = RC.FAMILIES
SIGMA = RC.SIGMA

AXIS_SIZES = [1, 5, 13]        # the axis identity of §13.1 on the CPU (the GPU takes every size)
CHAIN_VIEW = (0.5, (9, 17))    # (step, image) of the decomposed cases: rays all over the bounding sphere, 6 tiles

CLOSED_KINDS = ("zero", "half", "opaque")
CLOSED_VIEW = (0, 1.0, (9, 17))  # (direction, step, image) of the oblique frame of the closed family

Case = namedtuple("Case", "family N dtype direction step image emit")


def case_id(c):
    return (f"{c.family}-N{c.N}-{dname(c.dtype)}-{DIR_IDS[c.direction]}-s{c.step}-{c.image[0]}x{c.image[1]}-"
            f"{'emit' if c.emit else 'plain'}")


def big_image(N):
    return (N + 3, N)


def _cases():
    out, i = [], 0
    for N in SIZES:
        for dtype in DTYPES:
            for f, family in enumerate(FAMILIES):
                for d in range(len(DIRECTIONS)):
                    if N >= 64 and (d + f) % 3:  # the large sizes: each direction with one family
                        continue
                    images = FIXED_IMAGES + [big_image(N)]
                    out.append(Case(family, N, dtype, d, STEPS[i % 3], images[i % 7], bool((i // 4) % 2)))
                    i += 1  # (3 steps, 7 images: every pairing within 21 cases)
            for d in range(len(DIRECTIONS)):
                family = FAMILIES[d % 3] if N >= 13 else "random"
                for emit in ((True, False) if d == 0 else (bool(d % 2),)):
                    out.append(Case(family, N, dtype, d, 0.5, big_image(N), emit))
    return out


CASES = _cases()


def cases_of(N, dtype):
    return [c for c in CASES if c.N == N and c.dtype is dtype]


@functools.lru_cache(maxsize=None)
def _inputs(family, N, dtype_name):
    dtype = np.dtype(dtype_name).type
    if family == "special":
        dens, emit, _ = RC.random_pair(N, dtype)
        rng = np.random.RandomState(RC.special_seed(N))
        dens = SC.wall_specials(SC.special_values(dens, rng), rng)
        emit = SC.wall_specials(SC.special_values(emit, rng, nonfinite=N >= 13), rng, nonfinite=N >= 13)
    else:
        dens, emit, _ = RC.inputs(family, N, dtype)
        if family == "random":
            S3.set_bnd(0, dens)
            S3.set_bnd(0, emit)
    dens.setflags(write=False)
    emit.setflags(write=False)
    return dens, emit


def inputs(family, N, dtype):
    """(dens, emit, sigma) of a family; the arrays are shared and read-only."""
    dens, emit = _inputs(family, N, np.dtype(dtype).name)
    return dens, emit, SIGMA


def frame(N, direction, step, image, sigma=SIGMA):
    d, up = DIRECTIONS[direction]
    return VR.view_frame(N, d, up, image[0], image[1], step, sigma)


def closed(kind, N, dtype, axis=0, from_high=0):
    """(dens, emit, sigma) of render_cases.closed, read-only."""
    dens, emit, sigma = RC.closed(kind, N, dtype, axis, from_high)
    dens.setflags(write=False)
    emit.setflags(write=False)
    return dens, emit, sigma


def closed_expected(kind, N, dtype, emit, axis, from_high):
    """The exact (C, Tr) of an axis frame on a closed input rendered with emission (§12.1), or None where §12.1 gives
    none (half with emission; half beyond the mantissa width)."""
    if kind == "zero":
        return np.zeros((N, N), dtype), np.ones((N, N), dtype)
    if kind == "opaque":
        return np.ascontiguousarray(RR.cells(emit, axis, N if from_high else 1)), np.zeros((N, N), dtype)
    return None


def half_expected(N, dtype):
    """half without emission: (1 - 2^-N, 2^-N) while N <= the mantissa width, else None."""
    T = np.dtype(dtype).type
    if N > np.finfo(dtype).nmant + 1:
        return None
    return np.full((N, N), T(1) - T(2.0) ** -N, dtype), np.full((N, N), T(2.0) ** -N, dtype)


def edge_frame(N, sigma=SIGMA):
    """Rays along k through the points (a + 1.5, b + 1.5): the last pixel column and row lie exactly on the faces
    x = N + 0.5 and y = N + 0.5 of the box, which are visited (the box is closed) and read the shell with weight 0.5."""
    return VR.Frame(np.array([1.5, 1.5, 1.0]), np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), N,
                    sigma, N, N)


def case_frame(c):
    return frame(c.N, c.direction, c.step, c.image)


@functools.lru_cache(maxsize=None)
def _reference(family, N, dtype_name, direction, step, image, emit):
    dens, em, _ = inputs(family, N, np.dtype(dtype_name).type)
    C, Tr = VR.render_view(dens, em if emit else None, frame(N, direction, step, image))
    C.setflags(write=False)
    Tr.setflags(write=False)
    return C, Tr


def reference(c):
    """(C, Tr) of a case by the numpy reference: computed once per process, read-only."""
    return _reference(c.family, c.N, np.dtype(c.dtype).name, c.direction, c.step, c.image, c.emit)


def check_conditions(c, C, Tr):
    """The conditions of the module docstring on the reference result (C, Tr) of case c."""
    fr = case_frame(c)
    if c.image != (1, 1):
        missed = VR.visit_counts(c.N, c.dtype, fr) == 0
        assert missed.any(), (case_id(c), "no pixel misses the box")
        uint = np.uint32 if c.dtype is np.float32 else np.uint64
        assert (Tr[missed].view(uint) == np.ones(1, c.dtype).view(uint)[0]).all(), (case_id(c), "a missed pixel's Tr is not 1")
        assert (C[missed].view(uint) == 0).all(), (case_id(c), "a missed pixel's C is not +0")
    if c.image != big_image(c.N) or c.step != 0.5:
        return
    with np.errstate(invalid="ignore"):
        partial = np.count_nonzero((Tr > 0) & (Tr < 1))
        opaque = np.count_nonzero(Tr == 0)
    touched = np.count_nonzero(VR.visit_counts(c.N, c.dtype, fr))
    if c.N >= 13 or (c.N == 5 and c.family == "random"):
        assert 2 * partial >= touched, (case_id(c), partial, touched)
    if c.N >= 5:
        assert opaque >= 1, (case_id(c), "no ray ends at Tr = 0")
    if c.family == "special":
        for img in (C, Tr):
            assert 4 * np.count_nonzero(np.isnan(img)) < img.size, (case_id(c), np.count_nonzero(np.isnan(img)))
