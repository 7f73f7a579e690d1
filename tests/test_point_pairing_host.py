"""The per-lane pairing of k_pairing_check (c-kzg-4844_amd/csrc/pairing_dev.hpp), compiled for the host by g++ into
libhost_shim.so, against the host pairing it restates (host_pairing.hpp): final exponentiation, Fp12 inverse, Miller
product and the two-pair verdict byte for byte, and the cyclotomic square against the plain one."""
import ctypes as C
import os
import random
import subprocess

import pytest

from conftest import ROOT, SHIM_SO

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
FP12 = 576


@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    for name in ("hs_pd_final_exp", "hs_pd_fp12_inv", "hs_pd_cyclotomic_sqr", "hs_pd_miller", "hs_pd_pairing_check"):
        assert hasattr(lib, name), name
    return lib


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


def test_final_exp_matches_host(h):
    rnd = random.Random(11)
    for _ in range(3):
        f = _fp12(rnd)
        assert _call(h.hs_pd_final_exp, f) == _call(h.hs_host_final_exp, f)


def test_fp12_mul_and_inverse_match_host(h):
    rnd = random.Random(12)
    for _ in range(4):
        a, b = _fp12(rnd), _fp12(rnd)
        assert _call(h.hs_pd_fp12_mul, a, b) == _call(h.hs_host_fp12_mul, a, b)
        ia = _call(h.hs_pd_fp12_inv, a)
        assert ia == _call(h.hs_host_fp12_inv, a)
        assert h.hs_pd_is_one(_call(h.hs_pd_fp12_mul, a, ia)) == 1
    assert h.hs_pd_is_one(_fp12(rnd)) == 0


def test_cyclotomic_square_is_the_square_on_cyclotomic_elements(h):
    rnd = random.Random(13)
    for _ in range(4):
        f = _fp12(rnd)
        a = _call(h.hs_pd_easy_part, f)
        assert _call(h.hs_pd_cyclotomic_sqr, a) == _call(h.hs_pd_fp12_sqr, a)
        # (and not on a general element: the test would be vacuous otherwise)
        assert _call(h.hs_pd_cyclotomic_sqr, f) != _call(h.hs_pd_fp12_sqr, f)


def test_two_pair_verdicts_match_host(h):
    rnd = random.Random(14)
    g2 = _g2(h, 1)
    for rep in range(4):
        a, b = rnd.randrange(1, R), rnd.randrange(1, R)
        q1 = _g2(h, b)
        # e([a]G1, [b]G2) * e([-ab]G1, G2) == 1; a wrong second point breaks it
        p1, good, bad = _g1(h, a), _g1(h, R - a * b % R), _g1(h, R - a * b % R + 1)
        cases = [(p1, q1, good, g2, 1), (p1, q1, bad, g2, 0), (p1, g2, good, q1, 0)]
        # infinity in either slot: the other factor alone decides
        cases += [(INF1, q1, INF1, g2, 1), (INF1, q1, good, g2, 0), (p1, q1, INF1, g2, 0),
                  (INF1, q1, _g1(h, 0), g2, 1)]
        for x1, y1, x2, y2, want in cases:
            assert h.hs_pd_pairing_check(x1, y1, x2, y2) == want
            assert h.hs_pairing_prepared(x1, y1, x2, y2) == want
            assert _call(h.hs_pd_miller, x1, y1, x2, y2) == _call(h.hs_host_miller, x1, y1, x2, y2)
