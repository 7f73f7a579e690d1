"""The references of tests/cell_locate_expect.py by a second route each, without a GPU; and that the stage shim exports
what tests/test_gpu_cell_locate_stages.py binds."""
import ctypes as C
import os
import random
import subprocess

import cell_locate_expect as cx
import poly_expect as px
import rlc_expect as rx
from conftest import ROOT
from rlc_expect import R

ROOTS = rx.roots_of_unity()


def test_coset_points_are_the_columns_slice_of_the_extended_domain():
    # position 64 c + i of the extended domain in bit-reversed order is w^brp13(64 c + i)
    for col in (0, 1, 77, 127):
        assert cx.coset_points(ROOTS, col) == [ROOTS[px.brp(64 * col + i, 13)] for i in range(64)]
        h = ROOTS[rx.brev7(col)]
        assert all(pow(x, 64, R) == pow(h, 64, R) == rx.coset_factor(ROOTS, col) for x in cx.coset_points(ROOTS, col))


def test_minus_interp_evaluates_back_to_minus_the_cell():
    rnd = random.Random(64)
    for col in (0, 1, 127, 90):
        for cls in range(len(px.VALUE_CLASSES)):
            cell = px.class_vector(rnd, cls, 64)
            mi = cx.minus_interp(cell, col, ROOTS)
            assert [px.horner(mi, x) for x in cx.coset_points(ROOTS, col)] == [(-v) % R for v in cell], (col, cls)


def test_cell_of_poly_and_minus_interp_are_inverse():
    rnd = random.Random(65)
    for col in (0, 5, 127):
        coeffs = [rnd.randrange(R) for _ in range(64)]
        cell = cx.cell_of_poly(coeffs, col, ROOTS)
        assert cx.minus_interp(cell, col, ROOTS) == [(-v) % R for v in coeffs]
        # the same cell by the definition of the forward transform on the coset-scaled coefficients
        h = ROOTS[rx.brev7(col)]
        scaled = [v * pow(h, k, R) % R for k, v in enumerate(coeffs)]
        assert cell == px.ntt(scaled, ROOTS, 6, True, False, False)


def test_p1_log_is_the_cell_check_of_a_true_opening():
    # p of degree < 128, I = p mod (x^64 - h^64), q = (p - I) / (x^64 - h^64): C - [I(s)] + [h^64] proof = [s^64] proof
    rnd = random.Random(66)
    s = rnd.randrange(R)
    for col in (0, 3, 127):
        h64 = rx.coset_factor(ROOTS, col)
        p = [rnd.randrange(R) for _ in range(128)]
        q = p[64:]
        interp = [(p[k] + h64 * p[64 + k]) % R for k in range(64)]
        assert cx.minus_interp(cx.cell_of_poly(p, col, ROOTS), col, ROOTS) == [(-v) % R for v in interp]
        lhs = cx.p1_log(px.horner(p, s), px.horner(q, s), px.horner(interp, s), col, ROOTS)
        assert lhs == pow(s, 64, R) * px.horner(q, s) % R


def test_digits_scalar():
    import g1_expect as gx
    for c in (8, 10, 12):
        twin = gx.twin_for(c)
        d = [0] * (2 * twin)
        d[0], d[twin], d[twin + 1] = 3, -2, 1
        assert cx.digits_scalar(d, c) == (3 * gx.LAMBDA - 2 + (1 << c)) % R


def test_stage_shim_exports():
    so = os.path.join(ROOT, "c-kzg-4844_amd", "libcell_locate_shim.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libcell_locate_shim.so"])
    lib = C.CDLL(so)
    for fn in ("cs_digits_per_cell", "cs_cell_interp_digits", "cs_cell_lhs"):
        assert hasattr(lib, fn), fn
    lib.cs_digits_per_cell.restype = C.c_size_t
    assert [lib.cs_digits_per_cell(c) for c in (8, 10, 12, 13)] == [32 * 64, 26 * 64, 22 * 64, 0]
