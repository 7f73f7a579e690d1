"""The G1 corpus of tests/g1_points.py (valid points, points outside G1 of every torsion order the cofactor allows, bad
encodings) pinned on the CPU before any GPU sees it: the independent Python model, the oracle's
bytes_to_kzg_commitment (src/common/bytes.c:81-95) and the product's host arithmetic (host shim: the decompression,
the host subgroup test of small batches, and the 28-bit-limb endomorphism test the device kernels inline) must all
put every entry in the class the corpus says."""
import ctypes as C
import os
import subprocess

import pytest

import g1_points as GP
from conftest import ORACLE_SO, ROOT, SHIM_SO

CORPUS = GP.corpus()


@pytest.fixture(scope="module")
def libs():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    o, h = C.CDLL(ORACLE_SO), C.CDLL(SHIM_SO)
    o.og1_in_subgroup.restype = C.c_bool
    o.og1_is_inf.restype = C.c_bool
    return o, h


def test_corpus_covers_every_class():
    labels = [e.label for e in CORPUS]
    assert len(set(labels)) == len(labels)
    kinds = {e.expected for e in CORPUS}
    assert kinds == {GP.VALID, GP.NOT_IN_G1, GP.BAD_ENCODING}
    for ell in GP.TORSION_PRIMES:
        pts = [e.point for e in CORPUS if e.label.startswith("T%d_" % ell)]
        assert len(pts) == 2 and pts[0] != pts[1]
        for pt in pts:   # order exactly ell
            assert pt is not GP.INF and GP.mul(pt, ell) is GP.INF
        q_t = GP.by_label("Q+T%d" % ell).point
        assert GP.mul(q_t, GP.R) is not GP.INF and GP.mul(GP.mul(q_t, GP.R), ell) is GP.INF


@pytest.mark.parametrize("entry", CORPUS, ids=[e.label for e in CORPUS])
def test_reference_oracle_and_host_shim_agree_with_the_corpus(libs, entry):
    o, h = libs
    assert GP.classify(entry.data) == entry.expected
    # the oracle: bytes_to_kzg_commitment's return code, then its two halves
    jac = C.create_string_buffer(144)
    rc = o.okzg_bytes_to_kzg_commitment(jac, entry.data)
    assert rc == (0 if entry.expected == GP.VALID else 1)
    aff = C.create_string_buffer(96)
    ost = o.og1_uncompress(aff, entry.data)
    assert (ost == 0) == (entry.expected != GP.BAD_ENCODING)
    if ost == 0:
        o.og1_from_affine(jac, aff)
        in_g1 = o.og1_is_inf(jac) or o.og1_in_subgroup(jac)
        assert in_g1 == (entry.expected == GP.VALID)
        if isinstance(entry.point, tuple):   # the oracle decodes to the model's point (Montgomery form, radix 2^384)
            r384 = pow(2, 384, GP.P)
            assert int.from_bytes(aff.raw[:48], "little") == entry.point[0] * r384 % GP.P
            assert int.from_bytes(aff.raw[48:], "little") == entry.point[1] * r384 % GP.P
    # the product's host code: decompression (g1.hpp), subgroup tests (host_pairing.hpp, g1_28.hpp)
    haff = C.create_string_buffer(96)
    hst = h.hs_g1_uncompress(haff, entry.data)
    assert (hst == 0) == (entry.expected != GP.BAD_ENCODING)
    if hst == 0:
        if ost == 0:
            assert haff.raw == aff.raw
        if entry.point is GP.INF:
            assert haff.raw == bytes(96)
        else:
            want = 1 if entry.expected == GP.VALID else 0
            assert h.hs_g1_in_subgroup_host(haff) == want
            assert h.hs_g1_in_subgroup28(haff) == want
