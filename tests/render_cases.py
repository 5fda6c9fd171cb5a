"""The sizes, decompositions, seeds and inputs of the volume rendering tests (docs/SPEC.md §12), shared by
tests/test_render_ref.py (CPU: the conditions below hold and every wrong variant of the reference is told from it on a
named case) and tests/test_render_gpu.py (GPU: every case against the reference in bits).

Sizes: shape_cases.SIZES — one cell, ragged and full waves, the 64-lane seam, a second tile of 64 rows / columns of the
row march and a second trip of every march. Nothing in a march depends on N beyond those seams.

Input families, each (dens, emit, sigma):
  random    density uniform in [-0.25, 1] with sigma = 4 (a ray without an opaque cell ends near Tr = 0.2), about one cell
            in 4 N raised to N (t = 4: opaque), emission uniform in [-1, 2]; shells zero.
  shells    `random` with the shell cells of both fields filled with random opaque densities / large emissions: a ray
            that reads index 0 or N + 1 shows.
  special   `random` with shape_cases.special_values and wall_specials planted in both fields (NaN, infinities, zeros of
            either sign, ties; on the first and last cell of a row and at cells 64 / 65). Below N = 5 the emission
            takes the zeros and ties only: one NaN or infinity of emission makes its whole ray's C a NaN, and on 4
            or 9 rays no seed in 3000 keeps that to fewer than a quarter of the pixels; the density keeps them all.
  closed    the §12.1 inputs: closed("zero"), closed("half"), closed("opaque").
Conditions, checked on the reference by check_conditions (CPU for every case, GPU again on the result it compares with):
at least half of the pixels have 0 < Tr < 1; from N = 5 up at least one ray meets an opaque cell and at least one meets
none; in the special family fewer than a quarter of the pixels of either image are NaN. The seeds below satisfy them for
every size, dtype, axis and direction (tests/test_render_ref.py::test_conditions_hold). One exception, by necessity: in
the special family the first condition holds from N = 5 up. At N = 1 the one cell of the grid holds a planted value —
a zero, a NaN or an infinity — whose Tr is exactly 1 or 0 by §12, and at N = 2 and 3 the plants (25 of them and runs)
cover the 8 and 27 cells likewise: no seed in 3000 leaves half the rays partly transparent. Those three sizes keep the
special family (the bits are compared) and its NaN condition."""
import numpy as np

import render_ref as RR
import shape_cases as SC
from shape_cases import DECOMPOSED, DTYPES, SIZES, dname  # noqa: F401  (re-exported: the tests take them from here)

SIGMA = 4.0
INNER = (slice(1, -1),) * 3
VIEWS = [(axis, high) for axis in (0, 1, 2) for high in (0, 1)]
VIEW_IDS = [f"{'ijk'[a]}{'-' if h else '+'}" for a, h in VIEWS]
FAMILIES = ("random", "shells", "special")

# seed of family `random` (and of what `shells` and `special` plant into it) per N: 1200 + N unless listed
RANDOM_SEEDS = {1: 1205, 2: 1203, 3: 1215}
# seed of the planted special values per N: 1700 + N unless listed
SPECIAL_SEEDS = {5: 3812}


def random_seed(N):
    return RANDOM_SEEDS.get(N, 1200 + N)


def special_seed(N):
    return SPECIAL_SEEDS.get(N, 1700 + N)


def random_pair(N, dtype, seed=None):
    rng = np.random.RandomState(random_seed(N) if seed is None else seed)
    T = np.dtype(dtype).type
    dens = np.zeros((N + 2,) * 3, dtype)
    emit = np.zeros((N + 2,) * 3, dtype)
    d = rng.uniform(-0.25, 1.0, (N,) * 3)
    d = np.where(rng.random_sample((N,) * 3) < 1.0 / (4 * N), float(N), d)
    dens[INNER] = d.astype(dtype)
    emit[INNER] = rng.uniform(-1.0, 2.0, (N,) * 3).astype(dtype)
    return dens, emit, T


def inputs(family, N, dtype, seed=None):
    """(dens, emit, sigma) of a family."""
    dens, emit, _ = random_pair(N, dtype, seed if family != "special" else None)
    if family == "shells":
        rng = np.random.RandomState(random_seed(N) + 5000)
        shell = np.ones(dens.shape, bool)
        shell[INNER] = False
        dens[shell] = rng.uniform(0.5 * N, float(N) + 1.0, dens.shape).astype(dtype)[shell]
        emit[shell] = rng.uniform(10.0, 20.0, dens.shape).astype(dtype)[shell]
    elif family == "special":
        rng = np.random.RandomState(special_seed(N) if seed is None else seed)
        dens = SC.wall_specials(SC.special_values(dens, rng), rng)
        emit = SC.wall_specials(SC.special_values(emit, rng, nonfinite=N >= 5), rng, nonfinite=N >= 5)
    else:
        assert family == "random", family
    return dens, emit, SIGMA


def half_density(N, dtype, sigma=SIGMA):
    """The d with s * d == 0.5 exactly in T (s = T(sigma) * h is a power of two only when N is): the quotient 0.5 / s or
    a neighbour of it."""
    T = np.dtype(dtype).type
    s = RR.scalar(N, dtype, sigma)
    d = T(0.5) / s
    for cand in (d, np.nextafter(d, T(0)), np.nextafter(d, T(np.inf)), np.nextafter(np.nextafter(d, T(0)), T(0)),
                 np.nextafter(np.nextafter(d, T(np.inf)), T(np.inf))):
        if s * cand == T(0.5):
            return cand
    raise AssertionError(f"no density with s * d == 0.5 at N = {N} {dname(dtype)}")


def closed(kind, N, dtype, axis=0, from_high=0):
    """(dens, emit, sigma) of a §12.1 closed form: "zero" density; "half": uniform, s * d = 0.5 exactly; "opaque": the
    `random` input with the first cell every ray of this view visits made opaque."""
    dens, emit, T = random_pair(N, dtype)
    if kind == "zero":
        dens[...] = 0
    elif kind == "half":
        dens[INNER] = half_density(N, dtype)
    else:
        assert kind == "opaque", kind
        RR.cells(dens, axis, N if from_high else 1)[...] = T(2 * N)
    return dens, emit, SIGMA


def check_conditions(family, N, dens, C, Tr):
    """The conditions of the module docstring on a reference result (C, Tr) of the density `dens`."""
    with np.errstate(invalid="ignore"):
        partial = np.count_nonzero((Tr > 0) & (Tr < 1))
    if family != "special" or N >= 5:
        assert 2 * partial >= Tr.size, (family, N, partial, Tr.size)
    if N >= 5:
        assert np.count_nonzero(Tr == 0) >= 1, (family, N, "no ray meets an opaque cell")
        assert partial >= 1, (family, N, "every ray meets an opaque cell")
    if family == "special":
        for img in (C, Tr):
            assert 4 * np.count_nonzero(np.isnan(img)) < img.size, (family, N, np.count_nonzero(np.isnan(img)))
