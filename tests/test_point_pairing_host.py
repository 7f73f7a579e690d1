"""The per-lane pairing of k_pairing_check -- the tower of c-kzg-4844_amd/csrc/tower.hpp with the bodies the device
takes (32-bit CIOS Fp, Karatsuba Fp2) and the selecting Miller product of pairing_dev.hpp, compiled for the host by g++
into libfield32_shim.so (-U__SIZEOF_INT128__) -- against the host's pairing in libhost_shim.so (the same tower on 64-bit
limbs with the lazily reduced Fp2 forms, host_pairing.hpp's branching Miller product): final exponentiation, Fp12
inverse, Miller product and the two-pair verdict byte for byte, and the cyclotomic square against the plain one."""
import ctypes as C
import os
import random
import subprocess

import pytest

import field_cases as fc
from conftest import ROOT, SHIM_SO
from test_field_corpora_cpu import FIELD32_SO, run_host

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
FP12 = 576


@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    for name in ("hs_host_final_exp", "hs_host_fp12_inv", "hs_host_fp12_mul", "hs_host_miller", "hs_pairing_prepared"):
        assert hasattr(lib, name), name
    return lib


class Pd:
    """the operations of field_test_ops.hpp in the 32-bit-body build, on one item of bytes"""

    def __init__(self):
        if not os.path.exists(FIELD32_SO):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libfield32_shim.so"])
        self.lib = C.CDLL(FIELD32_SO)
        self.lib.hs_field_ops.restype = C.c_char_p
        self.ops = fc.parse_ops(self.lib.hs_field_ops().decode())
        self.index = {name: k for k, (name, _, _) in enumerate(self.ops)}

    def __call__(self, name, *args):
        """args: bytes (an Fp12) or word lists (an affine point, a line table); the result as bytes"""
        k = self.index[name]
        as_words = lambda a: [int.from_bytes(a[4 * j:4 * j + 4], "little") for j in range(len(a) // 4)]
        item = [list(a) if isinstance(a, list) else as_words(a) for a in args]
        out = run_host(self.lib, k, self.ops[k], [tuple(item + [None] * (4 - len(item)))])
        return bytes(out)

    def is_one(self, f):
        return int.from_bytes(self("fp12_is_one", f), "little")

    def easy_part(self, f):
        """f^((p^6-1)(p^2+1)): an element of the cyclotomic subgroup"""
        a = self("fp12_mul", self("fp12_conj", f), self("fp12_inv", f))
        return self("fp12_mul", self("frobenius_2", a), a)


@pytest.fixture(scope="module")
def pd():
    return Pd()


def _fp12(rnd):
    # any 12 values below p are Montgomery representatives of some Fp12 element
    return b"".join(rnd.randrange(P).to_bytes(48, "little") for _ in range(12))


def _call(fn, *args, n=FP12):
    out = C.create_string_buffer(n)
    fn(out, *args)
    return out.raw


def _g1(h, k):
    g = C.create_string_buffer(144)
    h.hs_g1_generator(g)
    kk = (C.c_uint32 * 8)(*[((k % R) >> (32 * i)) & 0xffffffff for i in range(8)])
    return _call(h.hs_g1_mul, g, kk, 255, n=144)


def _g2(h, k):
    g = C.create_string_buffer(288)
    h.hs_g2_generator(g)
    kk = (C.c_uint32 * 8)(*[((k % R) >> (32 * i)) & 0xffffffff for i in range(8)])
    return _call(h.hs_g2_mul, g, kk, 255, n=288)


INF1 = bytes(144)


def test_final_exp_matches_host(h, pd):
    rnd = random.Random(11)
    for _ in range(3):
        f = _fp12(rnd)
        assert pd("final_exp", f) == _call(h.hs_host_final_exp, f)


def test_fp12_mul_and_inverse_match_host(h, pd):
    rnd = random.Random(12)
    for _ in range(4):
        a, b = _fp12(rnd), _fp12(rnd)
        assert pd("fp12_mul", a, b) == _call(h.hs_host_fp12_mul, a, b)
        ia = pd("fp12_inv", a)
        assert ia == _call(h.hs_host_fp12_inv, a)
        assert pd.is_one(pd("fp12_mul", a, ia)) == 1
    assert pd.is_one(_fp12(rnd)) == 0


def test_cyclotomic_square_is_the_square_on_cyclotomic_elements(pd):
    rnd = random.Random(13)
    for _ in range(4):
        f = _fp12(rnd)
        a = pd.easy_part(f)
        assert pd("cyclotomic_sqr", a) == pd("fp12_sqr", a)
        # (and not on a general element: the test would be vacuous otherwise)
        assert pd("cyclotomic_sqr", f) != pd("fp12_sqr", f)


def test_two_pair_verdicts_match_host(h, pd):
    rnd = random.Random(14)
    pi = fc.PairingInputs(h)
    g2 = _g2(h, 1)
    tg2 = pi.table(g2)
    for rep in range(4):
        a, b = rnd.randrange(1, R), rnd.randrange(1, R)
        q1 = _g2(h, b)
        tq1 = pi.table(q1)
        tables = {q1: tq1, g2: tg2}
        # e([a]G1, [b]G2) * e([-ab]G1, G2) == 1; a wrong second point breaks it
        p1, good, bad = _g1(h, a), _g1(h, R - a * b % R), _g1(h, R - a * b % R + 1)
        cases = [(p1, q1, good, g2, 1), (p1, q1, bad, g2, 0), (p1, g2, good, q1, 0)]
        # infinity in either slot: the other factor alone decides
        cases += [(INF1, q1, INF1, g2, 1), (INF1, q1, good, g2, 0), (p1, q1, INF1, g2, 0),
                  (INF1, q1, _g1(h, 0), g2, 1)]
        for x1, y1, x2, y2, want in cases:
            a1, a2 = pi.affine(x1), pi.affine(x2)
            assert int.from_bytes(pd("pairing_product_is_one", a1, a2, tables[y1], tables[y2]), "little") == want
            assert h.hs_pairing_prepared(x1, y1, x2, y2) == want
            got = pd("miller_product_tables", a1, a2, tables[y1], tables[y2])
            assert got == _call(h.hs_host_miller, x1, y1, x2, y2)
