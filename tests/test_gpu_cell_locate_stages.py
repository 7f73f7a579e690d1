"""The two stages ckzg_hip_verify_cell_kzg_proof_batch_locate adds in front of the point form's pipeline, read off the
device and compared exactly (libcell_locate_shim.so: tests/native/cell_locate_shim.hip linked with the product's own
objects, so the kernels are the product's binary code):

  * k_cell_interp_digits (and the three-pass A/B partner): the whole digit buffer with a guard region behind it; every
    coefficient's digits stand for minus the interpolation coefficient, a Python integer (tests/cell_locate_expect.py);
  * interpolation -> 64-term fixed-base sum -> k_cell_lhs over 64 chosen bases [s^k]G: P1_i as a point against an integer
    multiple of G (one scalar multiplication of the CPU oracle), for cells of polynomials with known coefficients, whose
    I(s) is Horner's rule and no transform.

After any non-zero return of a shim call every later test of the module fails at once without launching anything."""
import array
import ctypes as C
import os
import random
import subprocess

import pytest

import cell_locate_expect as cx
import g1_expect as gx
import poly_expect as px
import rlc_expect as rx
from conftest import ORACLE_SO, ROOT
from rlc_expect import R

pytestmark = pytest.mark.gpu

CELL_SHIM_SO = os.path.abspath(os.environ["CKZG_CELL_LOCATE_SHIM_SO"]) if os.environ.get("CKZG_CELL_LOCATE_SHIM_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "libcell_locate_shim.so")
GUARD = 0x5a
_broken = []


class Shim:
    def __init__(self, lib):
        self.lib = lib

    def call(self, fn, *args):
        if _broken:
            pytest.fail("an earlier shim call failed (%s): nothing more is launched" % _broken[0])
        rc = getattr(self.lib, fn)(*args)
        if rc != 0:
            _broken.append("%s -> %d" % (fn, rc))
            pytest.fail(_broken[0])


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(CELL_SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libcell_locate_shim.so"])
    lib = C.CDLL(CELL_SHIM_SO)
    lib.cs_cell_interp_digits.restype = C.c_int
    lib.cs_cell_lhs.restype = C.c_int
    lib.cs_digits_per_cell.restype = C.c_size_t
    return Shim(lib)


@pytest.fixture(scope="module")
def roots():
    return rx.roots_of_unity()


@pytest.fixture(scope="module")
def src():
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    return gx.G1Source(C.CDLL(ORACLE_SO))


def _cells(rnd, n):
    """(cell values, column) per cell: all zero, all R - 1, one non-zero element at position 0 / at position 63, random;
    columns 0, 1, 127, 127 again, then random ones"""
    out = []
    for i in range(n):
        kind = i % 5
        if kind == 0:
            cell = [0] * 64
        elif kind == 1:
            cell = [R - 1] * 64
        elif kind == 2:
            cell = [rnd.randrange(1, R)] + [0] * 63
        elif kind == 3:
            cell = [0] * 63 + [rnd.randrange(1, R)]
        else:
            cell = [rnd.randrange(R) for _ in range(64)]
        out.append((cell, (0, 1, 127, 127)[i // 5] if i < 20 else rnd.randrange(128)))
    # (i // 5 < 4 for i < 20: each of the first four columns sees every kind of cell)
    return out


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n,wbits", [(1, 8), (63, 8), (64, 8), (65, 8), (24, 10), (24, 12)])
def test_interpolation_digits(shim, roots, n, wbits, fused):
    rnd = random.Random(1000 * n + wbits)
    cells = _cells(rnd, n)
    per = shim.lib.cs_digits_per_cell(wbits)
    nwin, half = per // 64, 1 << (wbits - 1)
    assert nwin == 2 * gx.twin_for(wbits)
    guard = 4096
    buf = C.create_string_buffer(bytes([GUARD]) * (2 * (n * per + guard)), 2 * (n * per + guard))
    shim.call("cs_cell_interp_digits", buf, C.c_size_t(n * per + guard), rx.le32([v for cell, _ in cells for v in cell]),
              (C.c_uint32 * n)(*[c for _, c in cells]), rx.le32(roots), C.c_size_t(n), wbits, fused)
    assert buf.raw[2 * n * per:] == bytes([GUARD]) * (2 * guard), "the guard behind the digits was written"
    d = array.array("h")
    d.frombytes(buf.raw[:2 * n * per])
    assert max(abs(v) for v in d) <= half
    for i, (cell, col) in enumerate(cells):
        want = cx.minus_interp(cell, col, roots)
        got = [cx.digits_scalar([d[i * per + w * 64 + k] for w in range(nwin)], wbits) for k in range(64)]
        assert got == want, (i, col, i % 5)
    # all zero stays all zero; a single element v at position 0: coefficient k is -v / 64 h^-k
    assert all(v == 0 for v in d[:per])
    if n > 2:
        assert len({cx.digits_scalar([d[2 * per + w * 64 + k] for w in range(nwin)], wbits) * pow(roots[rx.brev7(cells[2][1])], k, R) % R
                    for k in range(64)}) == 1


@pytest.mark.parametrize("fused,wbits", [(1, 10), (0, 10), (1, 8)])
def test_left_hand_points(shim, roots, src, fused, wbits):
    """wbits = 10: the width of the product's table"""
    rnd = random.Random(7594 + fused + wbits)
    n, nc = 65, 3
    s = rnd.randrange(2, R)
    mono = b"".join(src.raw(pow(s, k, R)) for k in range(64))
    a = [rnd.randrange(1, R), 0, rnd.randrange(1, R)]          # the commitments' logarithms (one is infinity)
    b = [rnd.randrange(1, R) for _ in range(n)]                # the proofs'
    b[5] = 0
    col = [(0, 1, 127, 127)[i] if i < 4 else rnd.randrange(128) for i in range(n)]
    commit = [i % nc for i in range(n)]
    polys = []
    for i in range(n):
        kind = i % 4
        polys.append([0] * 64 if kind == 0 else [rnd.randrange(R)] + [0] * 63 if kind == 1 else
                     [0] * 63 + [rnd.randrange(1, R)] if kind == 2 else [rnd.randrange(R) for _ in range(64)])
    cells = [cx.cell_of_poly(polys[i], col[i], roots) for i in range(n)]
    st_dec, st_sub, cell_bad = bytearray(n + nc), bytearray(n + nc), [0] * n
    # invalid items: a proof that did not decompress, one outside the subgroup, a column of 128, a flagged cell
    st_dec[9] = 1
    st_sub[63] = 1
    col[64] = 128
    cell_bad[10] = 1
    st_sub[n + 2] = 1   # ... and a commitment outside the subgroup: every item that names it
    invalid = {9, 63, 64, 10} | {i for i in range(n) if commit[i] == 2}
    pts = b"".join(src.raw(v) for v in b) + b"".join(src.raw(v) for v in a)
    lhs = C.create_string_buffer(bytes([GUARD]) * (192 * (n + 1)), 192 * (n + 1))
    negp = C.create_string_buffer(bytes([GUARD]) * (96 * (n + 1)), 96 * (n + 1))
    bad = C.create_string_buffer(bytes([GUARD]) * (n + 1), n + 1)
    shim.call("cs_cell_lhs", lhs, negp, bad, pts, bytes(st_dec), bytes(st_sub), rx.le32([v for cell in cells for v in cell]),
              (C.c_uint32 * n)(*col), (C.c_uint32 * n)(*commit), (C.c_uint32 * n)(*cell_bad), mono, rx.le32(roots), C.c_size_t(n),
              C.c_size_t(nc), wbits, fused)
    assert lhs.raw[192 * n:] == bytes([GUARD]) * 192 and negp.raw[96 * n:] == bytes([GUARD]) * 96 and bad.raw[n:] == bytes([GUARD])
    for i in range(n):
        got, got_np = lhs.raw[192 * i:192 * i + 192], negp.raw[96 * i:96 * i + 96]
        if i in invalid:
            assert bad.raw[i] == 1 and got == gx.ZERO_XYZZ and got_np == gx.ZERO_AFFINE, i
            continue
        assert bad.raw[i] == 0, i
        want = cx.p1_log(a[commit[i]], b[i], px.horner(polys[i], s), col[i], roots)
        assert gx.xyzz_is(got, src.raw(want)), (i, col[i], i % 4)
        assert gx.affine_point(got_np) == gx.affine_point(src.raw(-b[i])), i
