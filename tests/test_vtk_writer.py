"""VTK frame writer parity: fluidsolvergpu_amd/csrc/sf_vtk.cpp vs the reference's visit_writer.

Pinned two ways: (1) byte-equality with tests/golden/vtk/*.vtk, files written by the REFERENCE binary
(tests/golden/make_vtk_golden.py); (2) on seeded random cases, the SHA-256 and size of what the reference binary
wrote for them (tests/golden/vtk_random_sha256.json, same generator) and, when oracle/_ref is present,
byte-equality with the reference writing the same case in this process."""
import hashlib
import json
import os

import pytest

import ref_writer
import vtk_cases
from fluidsolvergpu_amd import vtk as sfvtk

GOLD = os.path.join(os.path.dirname(__file__), "golden", "vtk")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
RANDOM = json.load(open(os.path.join(os.path.dirname(GOLD), "vtk_random_sha256.json")))

# hashes of files produced by the compiled reference writer.
SURVEY_SHA = {
    "reg_ascii.vtk": "268453522d9d882bf4c933f1f1693a94f53ae207147aecd560ab782b1d1d8a56",
    "reg_bin.vtk": "95cc91b9b4306210097be2d7960e73963efdeaa6094bf7b8ca8aae7cd7b04e96",
    "pt_ascii.vtk": "e1c2d6bfdde7c319c2aaa9dbe963c8dfc50c7d4b4c65709ad06ec14185ee3634",
}


class _Product:
    """Adapts the package functions to the (…, vars_) calling convention of vtk_cases.run_case."""

    def __getattr__(self, name):
        return getattr(sfvtk, name)


class _ProductMangled(ref_writer.Writer):
    """Calls libsfvtk.so through the reference's C++-linkage names (drop-in link check)."""

    def __init__(self):
        super().__init__(os.path.join(os.path.dirname(sfvtk.__file__), "libsfvtk.so"))


@pytest.mark.parametrize("case", vtk_cases.cases(), ids=lambda c: c[0])
def test_matches_golden(case, tmp_path):
    path = vtk_cases.run_case(_Product(), case, str(tmp_path))
    got = open(path, "rb").read()
    want = open(os.path.join(GOLD, os.path.basename(path)), "rb").read()
    assert got == want
    assert hashlib.sha256(got).hexdigest() == MANIFEST[os.path.basename(path)]["sha256"]


def test_golden_matches_survey_hashes():
    for name, sha in SURVEY_SHA.items():
        assert MANIFEST[name]["sha256"] == sha
        assert hashlib.sha256(open(os.path.join(GOLD, name), "rb").read()).hexdigest() == sha


@pytest.mark.parametrize("case", vtk_cases.cases()[:6], ids=lambda c: c[0])
def test_cxx_linkage_names_are_drop_in(case, tmp_path):
    """The reference's mangled C++ names resolve in libsfvtk.so and write the same bytes."""
    path = vtk_cases.run_case(_ProductMangled(), case, str(tmp_path))
    assert open(path, "rb").read() == open(os.path.join(GOLD, os.path.basename(path)), "rb").read()


def _same_as_reference(key, write, tmp_path):
    """Writes the case with libsfvtk.so through `write(writer, path)`; its bytes must be those the reference wrote."""
    mine = str(tmp_path / "mine.vtk")
    write(sfvtk, mine)
    data = open(mine, "rb").read()
    assert len(data) == RANDOM[key]["bytes"] and hashlib.sha256(data).hexdigest() == RANDOM[key]["sha256"], key
    if ref_writer.available():
        ref = str(tmp_path / "ref.vtk")
        write(ref_writer.Writer(), ref)
        assert open(ref, "rb").read() == data


@pytest.mark.parametrize("seed", vtk_cases.RANDOM_SEEDS)
@pytest.mark.parametrize("ub", [0, 1])
def test_random_regular_mesh_vs_live_reference(seed, ub, tmp_path):
    args = vtk_cases.random_regular_case(seed, ub)
    _same_as_reference(vtk_cases.random_case_key(seed, ub), lambda w, p: w.write_regular_mesh(p, *args), tmp_path)


def test_float_formatting_vs_live_reference(tmp_path):
    """%20.12e of 200k random bit patterns (all exponents, denormals, inf/nan) — to_chars == printf."""
    args = vtk_cases.float_bits_case()
    _same_as_reference(vtk_cases.FLOAT_BITS_KEY, lambda w, p: w.write_point_mesh(p, *args), tmp_path)


def test_unwritable_path_raises(tmp_path):
    with pytest.raises(OSError):
        sfvtk.write_regular_mesh(str(tmp_path / "no_such_dir" / "x.vtk"), 0, [2, 2, 2], 0, [], [], [], [])


def test_extension_rule(tmp_path):
    """'.vtk' is appended only if the name does not already contain it (visit_writer.cpp:136-143)."""
    sfvtk.write_regular_mesh(str(tmp_path / "frame"), 1, [2, 2, 2], 0, [], [], [], [])
    sfvtk.write_regular_mesh(str(tmp_path / "a.vtk.bak"), 1, [2, 2, 2], 0, [], [], [], [])
    assert (tmp_path / "frame.vtk").exists() and (tmp_path / "a.vtk.bak").exists()
