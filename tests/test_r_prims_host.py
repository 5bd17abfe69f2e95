"""CPU: Mode R's primitive tests as the product's host code computes them (gi_math.h compiled by g++:
make_tri + tri_hit(TriRec), tri_hit_corners, box_hit, the OR of the four box_hit_part parts, sphere_hit)
against the COMPILED REFERENCE on the adversarial records of tests/r_prims_cases.py.

The chain, asserted in this order per kind (oracle_util.prims_expected, then assert_prims_equal):
  1. the generator's sha256 equals the one in tests/golden/adv_<kind>.npz (the inputs are the fixture's);
  2. the oracle's own routines (gio_prims; they do not include gi_math.h) reproduce the fixture -- the
     reference's hit bits, per-class hit counts, the sha256 of P|N per block of 512 cases, the stored samples;
  3. the product's host output equals the oracle's on every case: hit exactly, P and N bit for bit.
Nothing is excluded and there is no tolerance.  tests/test_gpu_r_prims.py makes the same assertions of the
device.  The program may also be built with -fsanitize=address,undefined and run stand-alone."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_util as U

OUT = np.dtype([("hit", "<i4"), ("hit2", "<i4"), ("pn", "<f8", 6)])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("r_prims") / "r_prims_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-I" + os.path.join(U.ROOT, "2019global_amd", "csrc"), "-o", exe,
                    os.path.join(U.ROOT, "tests", "cpp", "r_prims_check.cpp")], check=True)
    return exe


def run_checker(exe, kind, recs, tmp_path):
    rp, op = str(tmp_path / "r.bin"), str(tmp_path / "o.bin")
    with open(rp, "wb") as f:
        f.write(struct.pack("<i", recs.shape[0]))
        f.write(np.ascontiguousarray(recs, "<f8").tobytes())
    out = subprocess.run([exe, kind, rp, op], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    a = np.fromfile(op, dtype=OUT)
    assert a.shape[0] == recs.shape[0]
    return a


@pytest.mark.parametrize("kind", ["tris", "boxes", "spheres"])
def test_host_primitives_equal_the_reference(kind, checker, tmp_path):
    e = U.prims_expected(kind)   # assertions 1 and 2
    a = run_checker(checker, kind, e["recs"], tmp_path)
    if kind == "tris":
        U.assert_prims_equal(kind, "make_tri + tri_hit(TriRec)", a["hit"], a["pn"])
        U.assert_prims_equal(kind, "tri_hit_corners", a["hit2"])
    elif kind == "boxes":
        U.assert_prims_equal(kind, "box_hit", a["hit"])
        U.assert_prims_equal(kind, "OR of the box_hit_part parts", a["hit2"])
    else:
        U.assert_prims_equal(kind, "sphere_hit", a["hit"], a["pn"])


def test_class_sizes():
    """The floors the classes were sized to: 240,000 triangle, 60,000 box and 60,000 sphere cases."""
    import r_prims_cases as C
    for kind, floor in (("tris", 240000), ("boxes", 60000), ("spheres", 60000)):
        assert C.cases(kind)[0].shape[0] >= floor
