"""Every operation of c-kzg-4844_amd/csrc/field_test_ops.hpp as g++ builds it (libhost_shim.so: hs_field_run), on the
corpora of tests/field_cases.py against their exact references: Mont<Fp> / Mont<Fr> at the edge values, Fr29 on lazily
reduced operands at the bounds fr29.hpp states, the safegcd inversions on inputs chosen as the integer that reaches the
divsteps, and the pairing tower of tower.hpp against the Python tower of tests/tower_ref.py, which shares no code
with it.  This validates the corpora and the references without a GPU; tests/test_gpu_fields.py runs
the same lists through the device build.

Two host builds run every list: libhost_shim.so, where g++ takes the 64-bit-limb bodies of Mont's add / sub / mul, and
libfield32_shim.so (tests/native/field32_shim.cpp, -U__SIZEOF_INT128__), where it takes the 32-bit CIOS bodies that
the device compiler takes -- so a wrong carry there shows without a GPU, the tower on top of it included.  The tower's
Fp2 product and square differ the same way: the lazily reduced 64-bit forms in the first build, Karatsuba in the
second."""
import ctypes as C
import os
import subprocess

import pytest

import field_cases as fc
from conftest import ROOT, SHIM_SO
from test_gpu_dev_arith import DEV_SHIM_SO

PKG = os.path.join(ROOT, "c-kzg-4844_amd")
# CKZG_FIELD32_SO: another build of the 32-bit-body shim (the way conftest.py takes CKZG_SHIM_SO)
FIELD32_SO = os.path.abspath(os.environ["CKZG_FIELD32_SO"]) if os.environ.get("CKZG_FIELD32_SO") else \
    os.path.join(PKG, "csrc", "libfield32_shim.so")


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "csrc/libhost_shim.so"])
    h = C.CDLL(SHIM_SO)
    h.hs_field_ops.restype = C.c_char_p
    return h


@pytest.fixture(scope="module")
def shim32():
    if not os.path.exists(FIELD32_SO):
        subprocess.check_call(["make", "-C", PKG, "csrc/libfield32_shim.so"])
    h = C.CDLL(FIELD32_SO)
    h.hs_field_ops.restype = C.c_char_p
    return h


def _ops(h):
    return fc.parse_ops(h.hs_field_ops().decode())


def run_host(h, k, op, items):
    name, widths, shared = op
    a, b, c, d = [(C.c_uint32 * len(buf))(*buf) for buf in fc.pack(items, widths, shared)]
    out = (C.c_uint32 * (widths[0] * len(items)))()
    assert h.hs_field_run(k, out, a, b, c, d, len(items)) == 0
    return out


def test_required_operations_are_listed(shim):
    ops = _ops(shim)
    names = [name for name, _, _ in ops]
    assert len(set(names)) == len(names)
    for want in fc.REQUIRED_OPS:
        assert want in names, want
    for name, widths, shared in ops:
        assert 0 < widths[0] <= 144 and max(widths[1:3]) <= 144, name
        assert shared == (1 if name in fc.PAIRING_OPS else 0), name
    assert shim.hs_field_run(len(ops), None, None, None, None, None, 1) == 1     # a number past the list is refused


def test_device_shim_lists_the_same_operations(shim, shim32):
    assert shim32.hs_field_ops() == shim.hs_field_ops()
    if not os.path.exists(DEV_SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "-j", "3", "libdev_shim.so"])
    d = C.CDLL(DEV_SHIM_SO)
    d.ds_dev_field_ops.restype = C.c_char_p
    want = shim.hs_field_ops()
    assert want and d.ds_dev_field_ops() == want


def test_references_can_fail():
    """the checkers refuse a wrong word, the Python tower is a field (so its inverses-by-multiplying-back mean
    something), and the Fr29 reference's column walk does refuse an accumulator past 2^64 (limbs of three units)"""
    items, wants = fc.cached_corpus("fr_mul")
    bad = [w for row in wants for w in row]
    bad[8 * 3 + 2] ^= 1
    with pytest.raises(AssertionError):
        fc.check("fr_mul", wants, bad, 8)
    items, wants = fc.cached_corpus("fr29_inv")
    g = fc.val29(items[5][0])
    good = fc.limbs29(pow(g, -1, fc.R) * (1 << 522) % fc.R)
    wants[5](good)
    for wrong in (fc.limbs29(fc.val29(good) + 2 * fc.R), good[:3] + [good[3] ^ 1] + good[4:]):
        with pytest.raises(AssertionError):
            wants[5](wrong)
    tw = fc.tw
    a, b, c = fc._els(1, 12, 5)[2:5]
    assert tw.f12_mul(tw.f12_mul(a, b), c) == tw.f12_mul(a, tw.f12_mul(b, c)) and tw.f12_mul(a, b) == tw.f12_mul(b, a)
    assert tw.f12_mul(a, tw.F12_ONE) == a and tw.from_words(tw.to_words(a)) == a
    w = ((tw.F2_ZERO,) * 3, (tw.F2_ONE, tw.F2_ZERO, tw.F2_ZERO))
    assert tw.f12_mul(w, w) == (tw.V6, tw.F6_ZERO) and tw.f6_mul(tw.f6_mul(tw.V6, tw.V6), tw.V6) == (tw.XI, tw.F2_ZERO, tw.F2_ZERO)
    over = [3 << 29] * 9
    with pytest.raises(AssertionError):
        fc.mont29(over, over)


def _names():
    return [n for n in fc.REQUIRED_OPS if n not in fc.PAIRING_OPS]


@pytest.mark.parametrize("name", _names())
@pytest.mark.parametrize("build", ["limbs64", "limbs32"])
def test_host_form_on_the_corpora(shim, shim32, build, name):
    shim = shim32 if build == "limbs32" else shim
    ops = _ops(shim)
    ran = 0
    for k, op in enumerate(ops):
        if op[0] != name:
            continue
        items, wants = fc.cached_corpus(name)
        assert len(items) == len(wants) and len(items) >= 5
        out = run_host(shim, k, op, items)
        fc.check(name, wants, out, op[1][0])
        ran += 1
    assert ran == 1


def test_every_listed_operation_has_a_corpus(shim):
    for name, _, _ in _ops(shim):
        assert name in fc.REQUIRED_OPS, name + ": listed in field_test_ops.hpp but not run by the tests"


@pytest.mark.parametrize("build", ["limbs64", "limbs32"])
def test_miller_product_matches_host_and_the_python_tower(shim, shim32, build):
    """byte for byte host_pairing.hpp's value, and -- by the Python tower alone -- final_exp(miller([a]P, [b]Q)) ==
    final_exp(miller(P, Q))^(a b)"""
    lib = shim32 if build == "limbs32" else shim
    ops = _ops(lib)
    k = [n for n, _, _ in ops].index("miller_product_tables")
    items, wants, extra = fc.pairing_corpus("miller_product_tables", shim)
    out = run_host(lib, k, ops[k], items)
    fc.check("miller_product_tables", wants, out, 144)
    fc.check_miller_relation([list(out[144 * i:144 * (i + 1)]) for i in range(len(items))], extra)


@pytest.mark.parametrize("build", ["limbs64", "limbs32"])
def test_two_pair_verdicts(shim, shim32, build):
    lib = shim32 if build == "limbs32" else shim
    ops = _ops(lib)
    k = [n for n, _, _ in ops].index("pairing_product_is_one")
    items, wants, _ = fc.pairing_corpus("pairing_product_is_one", shim)
    assert len(items) == 37
    out = run_host(lib, k, ops[k], items)
    fc.check("pairing_product_is_one", wants, out, 1)
