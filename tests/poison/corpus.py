"""Inputs and expected values of the poison probes (tests/poison/driver.py), made WITHOUT the library under test: the
CPU oracle, the Python references of tests/, and two golden files the oracle made (tests/poison/make_golden.py).  Needs
no GPU: tests/test_gpu_poison.py builds the families' expected values once, in the pytest process, and hands them to the
children as a pickle."""
import ctypes as C
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
import coset_expect as E  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ORACLE_SO = os.path.join(ROOT, "oracle", "liboracle.so")
BLOB = 131072
CELL = 2048
G48 = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
INF48 = b"\xc0" + bytes(47)
ZS = E.ext_domain_points()                        # brp_roots_of_unity of the 8192-point domain, integers
EXT = [z.to_bytes(32, "big") for z in ZS]


def fr(v):
    return (v % R).to_bytes(32, "big")


def blob(i):
    """blob i of the corpus: 4096 canonical elements (the top byte is zero), different for every i"""
    return b"".join(b"\x00" + hashlib.sha256(b"poison %d %d" % (i, j)).digest()[:31] for j in range(4096))


def non_canonical(b, element=77):
    """the blob with one element replaced by the modulus"""
    return b[:32 * element] + R.to_bytes(32, "big") + b[32 * (element + 1):]


def bump(b32):
    """another canonical field element"""
    return fr(int.from_bytes(b32, "big") + 1)


def load_oracle():
    from oracle_binding import OracleKzg
    return OracleKzg(ORACLE_SO, precompute=0)


class OracleG1:
    """g1_t values (144 bytes, Jacobian) and their arithmetic through the oracle"""

    def __init__(self):
        self.o = o = C.CDLL(ORACLE_SO)
        o.og1_equal.restype = C.c_bool
        self.gen, self.inf = self.jac(G48), bytes(144)

    def jac(self, b48):
        aff, out = C.create_string_buffer(96), C.create_string_buffer(144)
        assert self.o.og1_uncompress(aff, b48) == 0
        self.o.og1_from_affine(out, aff)
        return out.raw

    def compress(self, p):
        out = C.create_string_buffer(48)
        self.o.og1_compress(out, p)
        return out.raw

    def add(self, a, b):
        r = C.create_string_buffer(144)
        self.o.og1_add(r, a, b)
        return r.raw

    def neg(self, a):
        r = C.create_string_buffer(144)
        self.o.og1_neg(r, a)
        return r.raw

    def mul(self, a, k):
        r = C.create_string_buffer(144)
        self.o.og1_mul_raw(r, a, (C.c_uint64 * 4)(*[(k >> (64 * i)) & (2 ** 64 - 1) for i in range(4)]), 255)
        return r.raw

    def eq(self, a, b):
        return bool(self.o.og1_equal(a, b))


def ladder_pair(g1, even, odd, e, c):
    """proof c at coset size 2^e from proofs 2c (even) and 2c + 1 (odd) at 2^(e-1): pi_e[c] = [1 / (2a)] (even - odd),
    a = x_c^(l/2)"""
    l = 1 << e
    a = pow(ZS[c * l], l // 2, R)
    diff = g1.add(g1.jac(even), g1.neg(g1.jac(odd)))
    return g1.compress(g1.mul(diff, pow(2 * a, -1, R)))


def ladder(g1, lower, e, first=0):
    """the proofs at coset size 2^e from those at 2^(e-1); lower[0] is proof 2 * first of that level"""
    return [ladder_pair(g1, lower[2 * i], lower[2 * i + 1], e, first + i) for i in range(len(lower) // 2)]


def golden_path(which):
    return os.path.join(TESTS, "golden", "poison_openings_b%d.bin" % which)


_GOLDEN = {}


def golden(which):
    """(the 8192 openings of coset size one, the 1024 of coset size 8) of blob(which), 48 bytes each"""
    if which not in _GOLDEN:
        raw = open(golden_path(which), "rb").read()
        assert len(raw) == (8192 + 1024) * 48
        _GOLDEN[which] = ([raw[48 * j:48 * j + 48] for j in range(8192)],
                          [raw[48 * (8192 + c):48 * (8192 + c) + 48] for c in range(1024)])
    return _GOLDEN[which]
