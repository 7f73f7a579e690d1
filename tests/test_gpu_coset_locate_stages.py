"""The two stages ckzg_hip_verify_coset_kzg_proof_batch_locate adds in front of the point form's pipeline, at every coset
size l = 2^e, read off the device and compared exactly (libcoset_locate_shim.so: tests/native/coset_locate_shim.hip
linked with the product's own objects, so the kernels are the product's binary code):

  * k_coset_item_interp_digits: the whole digit buffer with a guard region behind it; every coefficient's digits stand
    for minus the interpolation coefficient, a Python integer (tests/coset_verify_expect.py: interp_coeffs, by the
    definition of the inverse transform); item counts around a wave of 64 >> e items;
  * interpolation -> l-term fixed-base sum on a prefix of a 64-point table -> k_coset_item_lhs over chosen bases [s^k]G:
    P1_i as a point against an integer multiple of G (one scalar multiplication of the CPU oracle), for values of
    polynomials with known coefficients, whose I(s) is Horner's rule and no transform; in the launch form the product
    picks and in each of the narrow forms.

After any non-zero return of a shim call every later test of the module fails at once without launching anything."""
import array
import ctypes as C
import os
import random
import subprocess

import pytest

import coset_expect as E
import coset_locate_expect as X
import coset_verify_expect as V
import g1_expect as gx
import rlc_expect as rx
from conftest import ORACLE_SO, ROOT

pytestmark = pytest.mark.gpu

R = X.R
COSET_LOCATE_SHIM_SO = os.path.abspath(os.environ["CKZG_COSET_LOCATE_SHIM_SO"]) if os.environ.get("CKZG_COSET_LOCATE_SHIM_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "libcoset_locate_shim.so")
GUARD = 0x5a
ES = list(range(7))
ZS = E.ext_domain_points()
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
    if not os.path.exists(COSET_LOCATE_SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libcoset_locate_shim.so"])
    lib = C.CDLL(COSET_LOCATE_SHIM_SO)
    lib.cls_coset_interp_digits.restype = C.c_int
    lib.cls_coset_lhs.restype = C.c_int
    lib.cls_sum_lpv.restype = C.c_int
    lib.cls_digits_per_item.restype = C.c_size_t
    return Shim(lib)


@pytest.fixture(scope="module")
def roots():
    return rx.roots_of_unity()


@pytest.fixture(scope="module")
def src():
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    return gx.G1Source(C.CDLL(ORACLE_SO))


def _items(rnd, n, e):
    """(values, coset index) per item: all zero, all one, all R - 1, one non-zero value first / last, random; cosets 0, 1,
    m - 1, one past the range (clamped to m - 1 by the kernel), then random ones"""
    l, m = 1 << e, 8192 >> e
    out = []
    for i in range(n):
        kind = i % 6
        ys = [0] * l if kind == 0 else [1] * l if kind == 1 else [R - 1] * l if kind == 2 else \
            [rnd.randrange(1, R)] + [0] * (l - 1) if kind == 3 else [0] * (l - 1) + [rnd.randrange(1, R)] if kind == 4 else \
            [rnd.randrange(R) for _ in range(l)]
        out.append((ys, (0, 1, m - 1, m, m + 5)[i] if i < 5 else rnd.randrange(m)))
    return out


def _counts(e):
    w = 64 >> e
    return [n for n in (w - 1, w, w + 1, 3 * w + 1) if n > 0]


@pytest.mark.parametrize("e,n,wbits", [(e, n, 10) for e in ES for n in _counts(e)] + [(0, 65, 8), (3, 9, 8), (6, 2, 12)])
def test_interpolation_digits(shim, roots, e, n, wbits):
    rnd = random.Random(10000 * e + 10 * n + wbits)
    l = 1 << e
    items = _items(rnd, n, e)
    if n > 5:
        items = items[5:] + items[:5]   # the special cosets at the end as well: the tail of the last wave
    per = shim.lib.cls_digits_per_item(wbits, e)
    nwin, half = per // l, 1 << (wbits - 1)
    assert per and nwin == 2 * gx.twin_for(wbits)
    guard = 4096
    buf = C.create_string_buffer(bytes([GUARD]) * (2 * (n * per + guard)), 2 * (n * per + guard))
    shim.call("cls_coset_interp_digits", buf, C.c_size_t(n * per + guard), rx.le32([v for ys, _ in items for v in ys]),
              (C.c_uint32 * n)(*[c for _, c in items]), rx.le32(roots), C.c_size_t(n), e, wbits)
    assert buf.raw[2 * n * per:] == bytes([GUARD]) * (2 * guard), "the guard behind the digits was written"
    d = array.array("h")
    d.frombytes(buf.raw[:2 * n * per])
    assert max(abs(v) for v in d) <= half
    for i, (ys, c) in enumerate(items):
        want = X.minus_interp(ys, X.clamp(c, e), e)
        got = [X.digits_scalar([d[i * per + w * l + k] for w in range(nwin)], wbits) for k in range(l)]
        assert got == want, (i, c, ys[:2])
        if not any(ys):
            assert all(v == 0 for v in d[i * per:(i + 1) * per])
        if e == 0:
            assert got == [(-ys[0]) % R]


@pytest.mark.parametrize("lpv", [0, 4, 8, 16])
@pytest.mark.parametrize("e", ES)
def test_left_hand_points(shim, roots, src, e, lpv):
    """wbits = 10: the width of the product's table; lpv = 0: the form the product picks for this many items"""
    rnd = random.Random(7594 + 10 * e + lpv)
    l, m = 1 << e, 8192 >> e
    n, nc = 21 + (64 >> e), 3
    assert lpv or shim.lib.cls_sum_lpv(e, C.c_uint64(n)) == X.sum_lpv(e, n) == 64
    s = rnd.randrange(2, R)
    mono = b"".join(src.raw(pow(s, k, R)) for k in range(64))
    a = [rnd.randrange(1, R), 0, rnd.randrange(1, R)]          # the commitments' logarithms (one is infinity)
    b = [rnd.randrange(1, R) for _ in range(n)]                # the proofs'
    b[5] = 0
    idx = [(0, 1, m - 1, m - 1)[i] if i < 4 else rnd.randrange(m) for i in range(n)]
    commit = [i % nc for i in range(n)]
    polys = []
    for i in range(n):
        kind = i % 4
        polys.append([0] * l if kind == 0 else [rnd.randrange(R)] + [0] * (l - 1) if kind == 1 else
                     [0] * (l - 1) + [rnd.randrange(1, R)] if kind == 2 else [rnd.randrange(R) for _ in range(l)])
    vals = [[E.evaluate(polys[i], x) for x in ZS[idx[i] * l:(idx[i] + 1) * l]] for i in range(n)]
    st_dec, st_sub, val_bad = bytearray(n + nc), bytearray(n + nc), [0] * n
    # invalid items: a proof that did not decompress, one outside the subgroup, an index of m and a larger one, a flagged value
    st_dec[9] = 1
    st_sub[13] = 1
    idx[n - 1] = m
    idx[7] = m + 3
    val_bad[10] = 1
    st_sub[n + 2] = 1   # ... and a commitment outside the subgroup: every item that names it
    invalid = {9, 13, n - 1, 7, 10} | {i for i in range(n) if commit[i] == 2}
    pts = b"".join(src.raw(v) for v in b) + b"".join(src.raw(v) for v in a)
    lhs = C.create_string_buffer(bytes([GUARD]) * (192 * (n + 1)), 192 * (n + 1))
    negp = C.create_string_buffer(bytes([GUARD]) * (96 * (n + 1)), 96 * (n + 1))
    bad = C.create_string_buffer(bytes([GUARD]) * (n + 1), n + 1)
    shim.call("cls_coset_lhs", lhs, negp, bad, pts, bytes(st_dec), bytes(st_sub), rx.le32([v for ys in vals for v in ys]),
              (C.c_uint32 * n)(*idx), (C.c_uint32 * n)(*commit), (C.c_uint32 * n)(*val_bad), mono, rx.le32(roots), C.c_size_t(n),
              C.c_size_t(nc), e, 10, lpv)
    assert lhs.raw[192 * n:] == bytes([GUARD]) * 192 and negp.raw[96 * n:] == bytes([GUARD]) * 96 and bad.raw[n:] == bytes([GUARD])
    for i in range(n):
        got, got_np = lhs.raw[192 * i:192 * i + 192], negp.raw[96 * i:96 * i + 96]
        if i in invalid:
            assert bad.raw[i] == 1 and got == gx.ZERO_XYZZ and got_np == gx.ZERO_AFFINE, i
            continue
        assert bad.raw[i] == 0, i
        xl = pow(ZS[idx[i] * l], l, R)
        want = (a[commit[i]] - E.evaluate(polys[i], s) + xl * b[i]) % R
        assert want == X.p1_log(a[commit[i]], b[i], vals[i], idx[i], e, s)
        assert pow(V.root_of_unity(8192), V.shift_root(idx[i], e), R) == xl
        assert gx.xyzz_is(got, src.raw(want)), (i, idx[i], i % 4)
        assert gx.affine_point(got_np) == gx.affine_point(src.raw(-b[i])), i
