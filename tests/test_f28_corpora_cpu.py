"""The F28 field operations (c-kzg-4844_amd/csrc/fp28.hpp) as g++ builds them, at every bound combination the group
law instantiates (csrc/f28_test_ops.hpp), on raw limbs: worst-case lazily reduced operands (every limb at
LB * 2^28 - 1), limb mixes, the canonical edges, operands solved for chosen quotient digits and a random fill
(tests/arith_cases.py), against exact Python integers -- the product must equal (a b + q p) >> 392 limb for limb.
The reference also walks the columns with an unbounded accumulator and asserts that it stays below 2^64, which is
what the headers' static_asserts claim.  The device forms run the same corpora in test_gpu_dev_arith.py."""
import ctypes as C
import os
import subprocess

import pytest

import arith_cases as ac
from conftest import ROOT, SHIM_SO


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    h = C.CDLL(SHIM_SO)
    h.hs_f28_ops.restype = C.c_char_p
    return h


def _ops(h):
    return ac.parse_ops(h.hs_f28_ops().decode())


def test_required_instantiations_are_listed(shim):
    ops = _ops(shim)
    for want in ac.REQUIRED_OPS:
        assert want in ops, want
    assert {name for name, _ in ops} == ac.REQUIRED_KINDS
    assert len(set(ops)) == len(ops)
    assert shim.hs_f28_run(len(ops), None, None, None, None, None, 1) == 1   # a number past the list is refused


def test_reference_is_sound():
    """the exact formula and the column walk agree, the walk's accumulator really uses the top bit on worst-case
    operands (so the cases are at the edge the issue names), and the checker refuses a wrong limb"""
    op = ("mul", (4, 64, 4, 6))
    a, b = ac.operand_worst(4, 64), ac.operand_worst(4, 6)
    assert ac.value(a) <= 64 * ac.P < ac.value(a) + (1 << 364) and all(l == (4 << 28) - 1 for l in a[:13])
    t, q = ac.mont_exact([(a, b)])
    walked, peak = ac.replay_columns([(a, b)])
    assert walked == ac.canonical_limbs(t) and (1 << 63) < peak < (1 << 64)
    assert (t << 392) == ac.value(a) * ac.value(b) + q * ac.P and t < 2 * ac.P
    s = ac.operand_worst(4, 6)
    walked, peak = ac.replay_columns([(s, s)], square=True)
    assert walked == ac.canonical_limbs(ac.mont_exact([(s, s)])[0]) and (1 << 63) < peak < (1 << 64)
    good = ac.canonical_limbs(t)
    ac.check_field_result(op, (a, b), good)
    for j in (0, 7, 13):
        bad = list(good)
        bad[j] ^= 1
        with pytest.raises(AssertionError):
            ac.check_field_result(op, (a, b), bad)
    # a limb above the bound by one unit at the tightest instantiation would overflow: the budget is real
    over = [(5 << 28) - 1] * 13 + [0]
    assert ac.replay_columns([(over, over)])[1] >= 1 << 64


def test_every_class_is_present_for_every_bound(shim):
    for op in _ops(shim):
        cases = ac.field_cases(op)
        assert len(cases) >= ac.SUBSET_LEN and len({repr(c) for c in cases}) == len(cases), op   # a wave: 64 different cases
        if op[0] in ("mul", "sqr", "mul_add2"):
            b = ac.op_bounds(op)
            assert list(cases[0]) == [ac.operand_worst(*bd) for bd in b], op
            qs = {ac.mont_exact([(c[0], c[1 if len(c) > 1 else 0])] + ([(c[2], c[3])] if len(c) == 4 else []))[1]
                  for c in cases[:ac.SUBSET_LEN]}
            assert 0 in qs, op
            if op[0] != "sqr":
                assert ac.R392 - 1 in qs and ac.M28 in qs and (ac.M28 << (28 * 13)) in qs, op


def test_host_form_on_the_field_corpora(shim):
    ops = _ops(shim)
    peak = 0
    for k, op in enumerate(ops):
        cases, _, pk = ac.field_reference(op)
        a, b, c, d = ac.pack_operands(cases)
        out = (C.c_uint32 * (14 * len(cases)))()
        assert shim.hs_f28_run(k, out, a, b, c, d, len(cases)) == 0
        ac.check_field_run(op, out)
        peak = max(peak, pk)
    assert peak > 1 << 63    # some case drove the accumulator into its top bit


def test_host_form_of_the_plain_naf(shim):
    """naf2_128 (naf2.hpp) as g++ builds it: the digits are the non-adjacent form of k"""
    ks = ac.naf_scalars()
    n = len(ks)
    words = (C.c_uint32 * (4 * n))(*[(k >> (32 * j)) & 0xffffffff for k in ks for j in range(4)])
    out = (C.c_int8 * (ac.NAF2_LEN * n))()
    shim.hs_naf2_128(out, words, n)
    for i, k in enumerate(ks):
        ac.check_naf2(k, out[ac.NAF2_LEN * i:ac.NAF2_LEN * (i + 1)])
    top = [d for d in out[ac.NAF2_LEN * ks.index(2 ** 128 - 1):][:ac.NAF2_LEN]]
    assert top[0] == -1 and top[128] == 1 and not any(top[1:128])     # 2^128 - 1 = 2^128 - 2^0: the carry reaches digit 128
