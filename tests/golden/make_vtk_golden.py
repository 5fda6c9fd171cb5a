"""Generates tests/golden/vtk/*.vtk by running the REFERENCE's own visit_writer (compiled from
/root/reference/visit_writer.cpp into oracle/_ref by `make -C oracle ref`) on the deterministic cases
of tests/vtk_cases.py, and records the SHA-256 and size of what it writes for the random cases of
tests/test_vtk_writer.py in tests/golden/vtk_random_sha256.json (those files are too many or too large to commit).
Run where the reference sources are present:

    make -C oracle ref && python tests/golden/make_vtk_golden.py

The outputs are data (files written by the reference binary), committed as fixtures."""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_writer  # noqa: E402
import vtk_cases  # noqa: E402


def main():
    out_dir = os.path.join(HERE, "vtk")
    os.makedirs(out_dir, exist_ok=True)
    w = ref_writer.Writer()
    manifest = {}
    for case in vtk_cases.cases():
        path = vtk_cases.run_case(w, case, out_dir)
        data = open(path, "rb").read()
        manifest[os.path.basename(path)] = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
        print(f"{os.path.basename(path):24s} {len(data):7d} {manifest[os.path.basename(path)]['sha256']}")
    json.dump(manifest, open(os.path.join(out_dir, "MANIFEST.json"), "w"), indent=1, sort_keys=True)

    random = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "case.vtk")
        for seed in vtk_cases.RANDOM_SEEDS:
            for ub in (0, 1):
                w.write_regular_mesh(path, *vtk_cases.random_regular_case(seed, ub))
                random[vtk_cases.random_case_key(seed, ub)] = _digest(path)
        w.write_point_mesh(path, *vtk_cases.float_bits_case())
        random[vtk_cases.FLOAT_BITS_KEY] = _digest(path)
    json.dump(random, open(os.path.join(HERE, "vtk_random_sha256.json"), "w"), indent=1, sort_keys=True)


def _digest(path):
    data = open(path, "rb").read()
    return {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}


if __name__ == "__main__":
    main()
