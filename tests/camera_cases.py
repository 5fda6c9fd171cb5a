"""The sizes, cameras, inputs and conditions of the tests of perspective volume rendering (docs/SPEC.md §14), shared by
tests/test_render_camera_ref.py (CPU: the conditions hold, every wrong variant of the reference is told from it on a
named case) and tests/test_render_camera_gpu.py (GPU: every case against the reference in bits).

Inputs: the families of view_cases (random with set_bnd applied, shells, special) and its SIGMA, here the extinction per
cell length. Sizes: those of the §13 tests; N = 130 takes one frame per dtype. Images: view_cases.FIXED_IMAGES and
(N+3) x N, for the seams of the 8 x 8 pixel tile. Steps 0.5, 1 and 1.7 in depth.

Cameras (camera_frame of §14; c = (N+1)/2 the centre of the box):
  A  eye (c+0.2N, c, c-0.1N), target (c-N, c+0.3N, c+0.2N), tan 0.8: inside the box (t0 = 0), rays up and down
  B  eye (c-1.2N, c-0.7N, c+0.05N), target c, tan 0.7: outside, some pixels miss the box, rays up and down
  C  eye (c-0.45N, c-0.45N, c+0.02N), target (c+N, c+0.5N, c), tan 1.0: rays up and down
  U  eye (c+0.3N, c-0.2N, c-2N), target c, tan 0.4, up (0,1,0): every ray climbs (images no wider than 2.5 H)
  D  eye (c, c+0.1N, c+2.2N), target c, tan 0.4, up (0,1,0): every ray descends (likewise)
  K  eye (c, c, c-2N) looking along +k, up (0,1,0), tan 0.4: with odd W and H the centre pixel's r is exactly axial

The table CASES crosses sizes, dtypes and cameras and walks through the families, steps and images; every size from 5 up
also takes the (N+3) x N image at step 0.5 with cameras A, B, C, U and D, on which the conditions are stated.

Conditions (check_conditions; caps, not measurements), on the (N+3) x N image at step 0.5 from N = 13 up: at least half
of the pixels whose ray visits a sample end with 0 < Tr < 1; at least one ray ends at Tr = 0; in the special family
fewer than a quarter of the pixels of either image are NaN. On every image of cameras B and U of more than one pixel
column and row at least one pixel misses the box and is exactly (+0, 1)."""
import functools
from collections import namedtuple

import numpy as np

import render_camera_ref as CR
import view_cases as VC
from shape_cases import DTYPES, dname  # noqa: F401

SIZES = [1, 2, 3, 5, 13, 31, 34, 64, 65, 70]
ONE_FRAME = 130
DECOMPOSED = VC.DECOMPOSED + [(64, 4, "copy"), (40, 2, "rccl-self")]
STEPS = VC.STEPS
FIXED_IMAGES = VC.FIXED_IMAGES
FAMILIES = VC.FAMILIES
SIGMA = VC.SIGMA
CAMERAS = ("A", "B", "C", "U", "D", "K")
CONDITION_CAMERAS = ("A", "B", "C", "U", "D")
CHAIN_CAMERAS = ("A", "C", "U", "D")
MISSING = ("B", "U")           # cameras with a pixel that misses the box
CHAIN_VIEW = VC.CHAIN_VIEW     # (step, image) of the decomposed cases

Case = namedtuple("Case", "family N dtype camera step image emit")


def case_id(c):
    return f"{c.family}-N{c.N}-{dname(c.dtype)}-cam{c.camera}-s{c.step}-{c.image[0]}x{c.image[1]}-{'emit' if c.emit else 'plain'}"


def big_image(N):
    return (N + 3, N)


def camera(N, name):
    """(eye, target, up, tan_half_fov) of a camera."""
    c = (N + 1) / 2.0
    ctr = (c, c, c)
    return {
        "A": ((c + 0.2 * N, c, c - 0.1 * N), (c - N, c + 0.3 * N, c + 0.2 * N), (0, 0, 1), 0.8),
        "B": ((c - 1.2 * N, c - 0.7 * N, c + 0.05 * N), ctr, (0, 0, 1), 0.7),
        "C": ((c - 0.45 * N, c - 0.45 * N, c + 0.02 * N), (c + N, c + 0.5 * N, c), (0, 0, 1), 1.0),
        "U": ((c + 0.3 * N, c - 0.2 * N, c - 2.0 * N), ctr, (0, 1, 0), 0.4),
        "D": ((c, c + 0.1 * N, c + 2.2 * N), ctr, (0, 1, 0), 0.4),
        "K": ((c, c, c - 2.0 * N), ctr, (0, 1, 0), 0.4),
    }[name]


def frame(N, name, step, image, sigma=SIGMA):
    eye, target, up, tan = camera(N, name)
    fr = CR.camera_frame(N, eye, target, up, tan, image[0], image[1], step, sigma)
    assert fr is not None, (N, name, step, image)
    return fr


def _cases():
    out, i = [], 0
    for N in SIZES:
        for dtype in DTYPES:
            images = FIXED_IMAGES + [big_image(N)]
            for k, cam in enumerate(CAMERAS):
                if N >= 64 and (k + i) % 2:  # the large sizes: every other camera per dtype, all of them over the two
                    i += 1
                    continue
                image = images[i % 7]
                if cam == "K":  # odd extents: the centre pixel exists
                    image = [im for im in images if im[0] % 2 and im[1] % 2][i % 3 if N % 2 else i % 2]
                out.append(Case(FAMILIES[i % 3], N, dtype, cam, STEPS[(i // 3) % 3], image, bool((i // 2) % 2)))
                i += 1
            if N >= 5:
                for k, cam in enumerate(CONDITION_CAMERAS):
                    if N >= 64 and (k + (dtype is np.float64)) % 2:
                        continue
                    family = FAMILIES[(k + 1) % 3] if N >= 13 else "random"  # (special: B with emission, D without)
                    out.append(Case(family, N, dtype, cam, 0.5, big_image(N), bool(k % 2)))
    for dtype, cam in zip(DTYPES, ("A", "B")):
        out.append(Case("random", ONE_FRAME, dtype, cam, 1.0, (9, 17), dtype is np.float32))
    return out


CASES = _cases()
ALL_SIZES = SIZES + [ONE_FRAME]


def cases_of(N, dtype):
    return [c for c in CASES if c.N == N and c.dtype is dtype]


def inputs(family, N, dtype):
    """(dens, emit, sigma) of a family: view_cases' arrays, shared and read-only."""
    return VC.inputs(family, N, dtype)


def case_frame(c):
    return frame(c.N, c.camera, c.step, c.image)


@functools.lru_cache(maxsize=None)
def _reference(family, N, dtype_name, cam, step, image, emit):
    dens, em, _ = inputs(family, N, np.dtype(dtype_name).type)
    C, Tr = CR.render_camera(dens, em if emit else None, frame(N, cam, step, image))
    C.setflags(write=False)
    Tr.setflags(write=False)
    return C, Tr


def reference(c):
    """(C, Tr) of a case by the numpy reference: computed once per process, read-only."""
    return _reference(c.family, c.N, np.dtype(c.dtype).name, c.camera, c.step, c.image, c.emit)


def figures(c, C, Tr):
    """What the conditions are stated on: (visited pixels, partial, opaque, NaN of C, NaN of Tr, missed pixels)."""
    cnt = CR.visit_counts(c.N, c.dtype, case_frame(c))
    with np.errstate(invalid="ignore"):
        return (np.count_nonzero(cnt), np.count_nonzero((Tr > 0) & (Tr < 1)), np.count_nonzero(Tr == 0),
                np.count_nonzero(np.isnan(C)), np.count_nonzero(np.isnan(Tr)), np.count_nonzero(cnt == 0))


def check_conditions(c, C, Tr):
    """The conditions of the module docstring on the reference result (C, Tr) of case c."""
    fr = case_frame(c)
    on_big = c.image == big_image(c.N) and c.step == 0.5 and c.N >= 13
    misses = c.camera in MISSING and c.image[0] > 1 and c.image[1] > 1
    if not (on_big or misses):
        return
    cnt = CR.visit_counts(c.N, c.dtype, fr)
    if misses:
        missed = cnt == 0
        assert missed.any(), (case_id(c), "no pixel misses the box")
        uint = np.uint32 if c.dtype is np.float32 else np.uint64
        assert (Tr[missed].view(uint) == np.ones(1, c.dtype).view(uint)[0]).all(), (case_id(c), "a missed pixel's Tr is not 1")
        assert (C[missed].view(uint) == 0).all(), (case_id(c), "a missed pixel's C is not +0")
    if not on_big:
        return
    with np.errstate(invalid="ignore"):
        partial = np.count_nonzero((Tr > 0) & (Tr < 1))
        opaque = np.count_nonzero(Tr == 0)
    touched = np.count_nonzero(cnt)
    assert 2 * partial >= touched, (case_id(c), partial, touched)
    assert opaque >= 1, (case_id(c), "no ray ends at Tr = 0")
    if c.family == "special":
        for img in (C, Tr):
            assert 4 * np.count_nonzero(np.isnan(img)) < img.size, (case_id(c), np.count_nonzero(np.isnan(img)))
