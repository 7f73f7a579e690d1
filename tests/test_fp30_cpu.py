"""Fp on 13 signed 30-bit limbs (c-kzg-4844_amd/csrc/fp30.hpp) and the accumulate loop's mixed addition on it
(g1_30.hpp), compiled for the host into libhost_shim.so: limb-exact against Python integers, and the addition chain --
through entry, phi and exit -- against the 28-bit law it replaces in the throughput kernel."""
import ctypes as C
import os
import random
import subprocess

import pytest

from arith_cases import P, R
from conftest import ORACLE_SO, ROOT, SHIM_SO

N, W = 13, 30
HALF = 1 << 29
H13 = sum(HALF << (W * j) for j in range(N))        # value of the digit string (2^29, ..., 2^29), 13 digits
H12 = sum(HALF << (W * j) for j in range(N - 1))
PINV390 = pow(P, -1, 1 << 390)
I32x13 = C.c_int32 * N


@pytest.fixture(scope="module")
def libs():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    o, h = C.CDLL(ORACLE_SO), C.CDLL(SHIM_SO)
    o.og1_equal.restype = C.c_bool
    o.og1_is_inf.restype = C.c_bool
    return o, h


def value(limbs):
    return sum(int(v) << (W * j) for j, v in enumerate(limbs))


def out_limbs(v):
    """what a product or norm() leaves: limbs 0..11 balanced in [-2^29, 2^29), limb 12 the rest"""
    low = ((v + H12) % (1 << 360)) - H12
    t = low + H12
    return [((t >> (W * j)) & ((1 << W) - 1)) - HALF for j in range(N - 1)] + [(v - low) >> 360]


def model_product(s):
    """(s + q p) / 2^390 with the balanced quotient q = -s/p mod 2^390, digits in [-2^29, 2^29)"""
    q = (((-s * PINV390) % (1 << 390)) + H13) % (1 << 390) - H13
    t = s + q * P
    assert t % (1 << 390) == 0
    return out_limbs(t >> 390)


def column_product(a, b, c=None, d=None):
    """the column walk itself, digit by digit (checks model_product, and the 64-bit bound of every column)"""
    pl = out_limbs(P)
    ninv = (-pow(P, -1, 1 << W)) % (1 << W)
    q, r, acc = [], [], 0
    for k in range(2 * N - 1):
        lo, hi = max(0, k - (N - 1)), min(k, N - 1)
        acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        if c is not None:
            acc += sum(c[i] * d[k - i] for i in range(lo, hi + 1))
        up = 0
        if c is not None and 10 <= k <= 14:
            assert abs(acc) < 1 << 63
            up, acc = acc >> W, acc & ((1 << W) - 1)
        acc += sum(q[i] * pl[k - i] for i in range(lo, min(hi, len(q) - 1) + 1) if k - i >= 1)
        if k < N:
            qk = ((acc * ninv) % (1 << W) + HALF) % (1 << W) - HALF
            q.append(qk)
            acc += qk * pl[0]
        else:
            r.append(((acc % (1 << W)) + HALF) % (1 << W) - HALF)
            acc -= r[-1]
        assert abs(acc) < (1 << 63) - (1 << 60), k     # 2^60: room for the carry bias of two columns
        assert acc % (1 << W) == 0
        acc = (acc >> W) + up
    return r + [acc]


def rand_operand(rnd, vb):
    """normalised limbs of a random value of magnitude <= vb p"""
    return out_limbs(rnd.randrange(-vb * P, vb * P + 1))


def extreme_operands(vb):
    """the declared bounds, both signs: values at +-vb p, and limbs 0..11 all at +-2^29 (alternating too) under
    a top limb that keeps the value inside +-vb p"""
    out = [out_limbs(vb * P), out_limbs(-vb * P), [0] * N]
    for pattern in ([HALF] * 12, [-HALF] * 12, [HALF, -HALF] * 6, [-HALF, HALF] * 6):
        for target in (vb * P, -vb * P, 0):
            top = (target - value(pattern)) >> 360
            for t in (top, top + 1):
                cand = pattern + [t]
                if abs(value(cand)) <= vb * P and abs(t) <= HALF:
                    out.append(cand)
    assert len(out) >= 10
    return out


def call(h, name, *ops):
    r = I32x13()
    getattr(h, name)(r, *[I32x13(*x) for x in ops])
    return list(r)


def test_constants(libs):
    _, h = libs
    p, r392, r394, beta = I32x13(), I32x13(), I32x13(), I32x13()
    ninv = C.c_uint32()
    h.hs_fp30_consts(p, C.byref(ninv), r392, r394, beta)
    assert value(p) == P and all(abs(v) <= HALF for v in p)
    assert (ninv.value * P) % (1 << W) == (1 << W) - 1
    assert value(r392) == pow(2, 392, P) and value(r394) == pow(2, 394, P)
    b = value(beta) * pow(2, -390, P) % P
    assert b != 1 and pow(b, 3, P) == 1            # a primitive cube root of unity: beta
    # it is the beta of the 28-bit loop (the oracle has no such export; phi is pinned again by the chain test)
    for arr in (r392, r394, beta):
        assert all(abs(v) <= HALF for v in arr)


def test_model_is_the_column_walk():
    rnd = random.Random(30)
    for _ in range(40):
        a, b, c, d = (rand_operand(rnd, v) for v in (17, 17, 5, 5))
        assert column_product(a, b) == model_product(value(a) * value(b))
        assert column_product(a, b, c, d) == model_product(value(a) * value(b) + value(c) * value(d))
    # every limb at the bound, all signs aligned: the fullest columns the static_asserts admit
    for s in (1, -1):
        full = [HALF] * 12 + [0]
        neg = [s * v for v in full]
        column_product(full, neg)
        column_product(full, neg, full, neg)


def test_mul_sqr_mul_add2_norm_exact(libs):
    _, h = libs
    rnd = random.Random(31)
    e17, e18, e5 = extreme_operands(17), extreme_operands(18), extreme_operands(5)
    for k in range(10000 + len(e17) * len(e18)):
        if k < len(e17) * len(e18):
            a, b = e17[k % len(e17)], e18[k // len(e17)]
            b2 = e17[(k // len(e17)) % len(e17)]
            c, d = e5[k % len(e5)], e5[(k // 3) % len(e5)]
        else:
            a, b, b2, c, d = (rand_operand(rnd, v) for v in (17, 18, 17, 5, 5))
        got = call(h, "hs_fp30_mul", a, b)
        assert got == model_product(value(a) * value(b)), (a, b)
        assert abs(value(got)) <= P and all(abs(v) <= HALF for v in got)
        assert (value(got) << 390) % P == value(a) * value(b) % P
        got = call(h, "hs_fp30_sqr", a)
        assert got == model_product(value(a) ** 2), a
        got = call(h, "hs_fp30_mul_add2", a, b2, c, d)
        assert got == model_product(value(a) * value(b2) + value(c) * value(d)), (a, b2, c, d)
        assert abs(value(got)) <= P
        # norm on limbs of up to 3 * 2^29: sums and differences of three normalised operands
        s3 = [x + y - z for x, y, z in zip(a, b, c)]
        got = call(h, "hs_fp30_norm", s3)
        assert got == out_limbs(value(s3)), s3
        assert call(h, "hs_fp30_add", a, c) == [x + y for x, y in zip(a, c)]
        assert call(h, "hs_fp30_sub", a, c) == [x - y for x, y in zip(a, c)]
    for s in (3 * HALF, -3 * HALF):
        lim = [s] * 12 + [17 << 21]
        assert call(h, "hs_fp30_norm", lim) == out_limbs(value(lim))


def test_unpack_and_repack(libs):
    _, h = libs
    rnd = random.Random(32)
    edge = [0, 1, P - 1, (1 << 381) - 1 if (1 << 381) - 1 < P else P - 2, sum(1 << (W * j + 29) for j in range(12))]
    edge += [sum(((1 << W) - 1) << (W * j) for j in range(12)), sum((HALF - 1) << (W * j) for j in range(12))]
    for k in range(2000):
        v = edge[k] if k < len(edge) else rnd.randrange(P)
        words = (C.c_uint32 * 12)(*[(v >> (32 * i)) & 0xffffffff for i in range(12)])
        r = I32x13()
        h.hs_fp30_unpack(r, words)
        assert value(r) == v and all(abs(x) <= HALF for x in r), v
        # a product's output (|value| <= p) -> 14 x 28-bit limbs of value + p, normalised
        a = rand_operand(rnd, 1) if k >= 4 else [out_limbs(P), out_limbs(-P), [0] * N, out_limbs(P - 1)][k]
        o = (C.c_uint32 * 14)()
        h.hs_fp30_to_f28(o, I32x13(*a))
        assert sum(int(x) << (28 * j) for j, x in enumerate(o)) == value(a) + P
        assert all(x < 1 << 28 for x in o)


def _omul(o, p, k):
    r = C.create_string_buffer(144)
    kk = (C.c_uint64 * 4)(*[(k >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])
    o.og1_mul_raw(r, p, kk, 255)
    return r


def _aff(o, p):
    a = C.create_string_buffer(96)
    o.og1_to_affine(a, p)
    return a.raw


@pytest.fixture(scope="module")
def base_points(libs):
    o, h = libs
    rnd = random.Random(33)
    g = C.create_string_buffer(144)
    h.hs_g1_generator(g)
    return [_omul(o, g, rnd.randrange(1, R)) for _ in range(300)]


def _chain(h, pts, signs, at_inf, phi_at, form):
    r = C.create_string_buffer(144)
    h.hs_g1_madd_alt_chain_form.restype = C.c_int
    met = h.hs_g1_madd_alt_chain_form(r, b"".join(pts), bytes(signs), bytes(at_inf), len(pts), phi_at, form)
    return r, met


def test_chain_of_300_matches_the_28_bit_law(libs, base_points):
    o, h = libs
    rnd = random.Random(34)
    pts = [_aff(o, p) for p in base_points]
    signs = [rnd.randrange(2) for _ in pts]
    at_inf = [0] * len(pts)
    for i in (0, 7, 150, 151, 299):
        at_inf[i] = 1                      # entries at infinity: first, in the middle, around phi, last
    for phi_at in (151, 1, 300, 1000):     # in the middle; before the first addition; after the last; never crossed
        ref, _ = _chain(h, pts, signs, at_inf, phi_at, 0)
        assert not o.og1_is_inf(ref)
        for form in (1, 2):
            got, met = _chain(h, pts, signs, at_inf, phi_at, form)
            assert met == 0
            assert _aff(o, got) == _aff(o, ref), (phi_at, form)
    # without phi (phi on an empty accumulator is skipped) the chain is the plain signed sum
    head = 40
    ref = C.create_string_buffer(144)
    for p, s, z in zip(base_points[:head], signs, at_inf):
        if z:
            continue
        q = C.create_string_buffer(144)
        q.raw = p.raw
        if s:
            o.og1_neg(q, q)
        o.og1_add(ref, ref, q)
    # phi_at = 0: applied while the accumulator is still empty
    got, met = _chain(h, pts[:head], signs[:head], at_inf[:head], 0, 1)
    assert met == 0 and o.og1_equal(got, ref)
    # everything skipped: infinity
    got, met = _chain(h, pts[:5], signs[:5], [1] * 5, 2, 1)
    assert met == 0 and o.og1_is_inf(got)


def test_equal_x_leaves_zz_zero_and_the_fallback_is_exact(libs, base_points):
    o, h = libs
    rnd = random.Random(35)
    head, tail = 11, 9
    pts = [_aff(o, p) for p in base_points[:head + tail]]
    signs = [rnd.randrange(2) for _ in pts]
    run = C.create_string_buffer(144)      # the running sum after `head` entries
    for p, s in zip(base_points[:head], signs):
        q = C.create_string_buffer(144)
        q.raw = p.raw
        if s:
            o.og1_neg(q, q)
        o.og1_add(run, run, q)
    for same in (True, False):             # acc + (same point): doubling;  acc + (-point): infinity
        for rest in (tail, 0):             # in the middle of a chain, and as its last step
            mid_sign = 0 if same else 1
            cp = pts[:head] + [_aff(o, run)] + pts[head:head + rest]
            cs = signs[:head] + [mid_sign] + signs[head:head + rest]
            zi = [0] * len(cp)
            n = len(cp)
            ref, _ = _chain(h, cp, cs, zi, n, 0)
            _, met = _chain(h, cp, cs, zi, n, 1)
            assert met == 1, (same, rest)
            got, met = _chain(h, cp, cs, zi, n, 2)
            assert met == 1
            if rest == 0 and not same:
                assert o.og1_is_inf(got) and o.og1_is_inf(ref)
            else:
                assert not o.og1_is_inf(ref)
                assert _aff(o, got) == _aff(o, ref), (same, rest)
            # and the plain group law agrees (phi at the end of the chain: compare before it by undoing nothing --
            # phi_at = n applies phi to the whole sum, so check the phi-free chain too)
            exp = C.create_string_buffer(144)
            exp.raw = run.raw
            if same:
                o.og1_dbl(exp, exp)
            else:
                o.og1_neg(exp, exp)
                o.og1_add(exp, exp, run)
            for p, s in zip(base_points[head:head + rest], signs[head:head + rest]):
                q = C.create_string_buffer(144)
                q.raw = p.raw
                if s:
                    o.og1_neg(q, q)
                o.og1_add(exp, exp, q)
            got0, met = _chain(h, cp, cs, zi, 0, 2)
            assert met == 1 and o.og1_equal(got0, exp), (same, rest)


def test_generated_includes_are_the_generators_output():
    import sys
    csrc = os.path.join(ROOT, "c-kzg-4844_amd", "csrc")
    for mode, name in (("consts", "fp30_consts.inc"), ("cols", "fp30_asm_cols.inc")):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fp30_asm.py"), mode],
                             capture_output=True, text=True, check=True).stdout
        with open(os.path.join(csrc, name)) as f:
            assert f.read() == out, "%s is stale: python tools/gen_fp30_asm.py %s > c-kzg-4844_amd/csrc/%s" % (name, mode, name)
