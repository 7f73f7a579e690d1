"""What the two stages of the cell form of the *_locate calls must produce, as Python integers
(tests/test_gpu_cell_locate_stages.py; second routes: tests/test_cell_locate_expect_cpu.py).  Nothing here reads the
library under test.

A cell of column c holds 64 evaluations in bit-reversed order: element i is the value at h w64^brp6(i), h = w^brev7(c)
the coset factor of the column and w64 = w^128.  Its interpolation polynomial I has degree < 64; the device writes the
digits of -I[k], and the left-hand point of the item's check is P1 = C - [I(s)]_1 + [h^64] proof."""
import g1_expect as gx
import poly_expect as px
from rlc_expect import R, brev7


def coset_points(roots, col):
    """where element i of a cell of column col is an evaluation: h w64^brp6(i)"""
    h = roots[brev7(col)]
    return [h * roots[128 * px.brp(i, 6)] % R for i in range(64)]


def minus_interp(cell, col, roots):
    """-I[k], k < 64: the inverse transform of fr_ntt_batch(.., 6, false, true, true) on the cell as it is stored, then
    coefficient k times (h^-1)^k, negated"""
    coef = px.ntt(list(cell), roots, 6, False, True, True)
    rb = brev7(col)
    return [(-coef[k] * roots[((8192 - rb) * k) % 8192]) % R for k in range(64)]


def cell_of_poly(coeffs, col, roots):
    """the cell of column col of a polynomial with the given (at most 64) coefficients: Horner at every coset point"""
    return [px.horner(coeffs, x) for x in coset_points(roots, col)]


def digits_scalar(d, c):
    """the scalar a digit string of one coefficient stands for: k1 + lambda k2"""
    k1, k2 = gx.digits_value(d, c)
    return (k1 + k2 * gx.LAMBDA) % R


def p1_log(a_commit, b_proof, poly_at_s, col, roots):
    """the discrete logarithm of P1 = C - [I(s)]G + [h^64] proof for C = [a]G, proof = [b]G and I(s) as an integer"""
    return (a_commit - poly_at_s + roots[64 * brev7(col)] * b_proof) % R
