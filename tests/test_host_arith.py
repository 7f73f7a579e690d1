"""The product's header-only arithmetic (c-kzg-4844_amd/csrc/field.hpp, g1.hpp, host_pairing.hpp),
compiled for the host by g++ into libhost_shim.so, against the oracle limb for limb.  The same
headers are what the HIP kernels inline, so this covers the device formulas without a GPU."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

import arith_cases as ac
from arith_cases import LAMBDA, P, R   # the case scripts are shared with the device tests (tests/arith_cases.py)
from conftest import ORACLE_SO, ROOT, SHIM_SO


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


def _buf(n):
    return C.create_string_buffer(n)


def test_field_ops_match(libs):
    o, h = libs
    rnd = random.Random(5)
    for name, nbytes, mod in (("fp", 48, P), ("fr", 32, R)):
        edge = [0, 1, mod - 1, mod - 2, (mod - 1) // 2]
        for op in ("mul", "add", "sub"):
            for k in range(300):
                a = edge[k % 5] if k < 25 else rnd.randrange(mod)
                b = edge[(k // 5) % 5] if k < 25 else rnd.randrange(mod)
                ab, bb = a.to_bytes(nbytes, "little"), b.to_bytes(nbytes, "little")
                r1, r2 = _buf(nbytes), _buf(nbytes)
                getattr(o, "o%s_%s" % (name, op))(r1, ab, bb)
                getattr(h, "hs_%s_%s" % (name, op))(r2, ab, bb)
                assert r1.raw == r2.raw, (name, op, a, b)
        for _ in range(4):
            a = rnd.randrange(1, mod).to_bytes(nbytes, "little")
            r1, r2 = _buf(nbytes), _buf(nbytes)
            getattr(o, "o%s_inv" % name)(r1, a)
            getattr(h, "hs_%s_inv" % name)(r2, a)
            assert r1.raw == r2.raw


def _omul(o, p, k):
    r = _buf(144)
    kk = (C.c_uint64 * 4)(*[(k >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])
    o.og1_mul_raw(r, p, kk, 255)
    return r


def test_g1_group_laws_match(libs):
    o, h = libs
    rnd = random.Random(7)
    g = _buf(144)
    h.hs_g1_generator(g)
    inf = _buf(144)
    for _ in range(6):
        k1, k2 = rnd.randrange(R), rnd.randrange(R)
        p1, p2 = _omul(o, g, k1), _omul(o, g, k2)
        ref = _buf(144)
        o.og1_add(ref, p1, p2)
        a1, a2 = _buf(96), _buf(96)
        o.og1_to_affine(a1, p1)
        o.og1_to_affine(a2, p2)
        for fn, arg in (("hs_g1_add_jac", p2), ("hs_g1_add_xyzz", p2), ("hs_g1_madd_xyzz", a2), ("hs_g1_madd_jac", a2)):
            r = _buf(144)
            getattr(h, fn)(r, p1, arg)
            assert o.og1_equal(r, ref), fn
        dbl = _buf(144)
        o.og1_dbl(dbl, p1)
        # the complete laws must take the doubling path when both inputs are the same point
        for fn, arg in (("hs_g1_add_jac", p1), ("hs_g1_add_xyzz", p1), ("hs_g1_madd_xyzz", a1), ("hs_g1_madd_jac", a1)):
            r = _buf(144)
            getattr(h, fn)(r, p1, arg)
            assert o.og1_equal(r, dbl), fn
        for fn in ("hs_g1_dbl_jac", "hs_g1_dbl_xyzz"):
            r = _buf(144)
            getattr(h, fn)(r, p1)
            assert o.og1_equal(r, dbl), fn
        # P + (-P) = infinity, infinity + P = P
        n1 = _buf(144)
        o.og1_neg(n1, p1)
        for fn in ("hs_g1_add_jac", "hs_g1_add_xyzz"):
            r = _buf(144)
            getattr(h, fn)(r, p1, n1)
            assert o.og1_is_inf(r), fn
            r = _buf(144)
            getattr(h, fn)(r, inf, p1)
            assert o.og1_equal(r, p1), fn
        kk = (C.c_uint32 * 8)(*[(k2 >> (32 * i)) & 0xffffffff for i in range(8)])
        r = _buf(144)
        h.hs_g1_mul(r, p1, kk, 255)
        ref3 = _omul(o, p1, k2)
        assert o.og1_equal(r, ref3)
        c1, c2 = _buf(48), _buf(48)
        o.og1_compress(c1, ref3)
        h.hs_g1_compress(c2, r)
        assert c1.raw == c2.raw
        u, a3 = _buf(96), _buf(96)
        assert h.hs_g1_uncompress(u, c1.raw) == 0
        o.og1_to_affine(a3, ref3)
        assert u.raw == a3.raw


# the 15 accept/reject encodings pinned by /root/reference/src/test/tests.c:551-747
G1_ENCODING_KATS = [
    ("a491d1b0ecd9bb917989f0e74f0dea0422eac4a873e5e2644f368dffb9a6e20fd6e10c1b77654d067c0618f6e5a7f79a", True),
    ("8123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef", False),
    ("8123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcde0", False),
    ("9a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab", False),
    ("9a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaac", False),
    ("c0" + "00" * 47, True),
    ("c01" + "0" * 93, False),
    ("80" + "00" * 47, False),
    ("0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef", False),
    ("c123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef", False),
    ("e0" + "00" * 47, False),
    ("e491d1b0ecd9bb917989f0e74f0dea0422eac4a873e5e2644f368dffb9a6e20fd6e10c1b77654d067c0618f6e5a7f79a", False),
]


def test_g1_encoding_kats_host_and_oracle(libs):
    o, h = libs
    o.og1_in_subgroup.restype = C.c_bool
    for hx, ok in G1_ENCODING_KATS:
        b = bytes.fromhex(hx)
        for lib, fn in ((h, "hs_g1_uncompress"), (o, "og1_uncompress")):
            a = _buf(96)
            rc = getattr(lib, fn)(a, b)
            valid = rc == 0
            if valid:
                j = _buf(144)
                o.og1_from_affine(j, a)
                valid = o.og1_is_inf(j) or o.og1_in_subgroup(j)
            assert valid == ok, (hx[:8], fn)


def test_pairing_and_sha(libs):
    o, h = libs
    g = _buf(144)
    g2 = _buf(288)
    h.hs_g1_generator(g)
    h.hs_g2_generator(g2)
    k = 0x1234567890abcdef1234567890abcdef % R
    kk = (C.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
    kg1 = _omul(o, g, k)
    kg2 = _buf(288)
    h.hs_g2_mul(kg2, g2, kk, 255)
    assert h.hs_pairings_verify(kg1, g2, g, kg2) == 1
    assert h.hs_pairings_verify(kg1, g2, kg1, kg2) == 0
    for n in (0, 1, 55, 56, 63, 64, 65, 119, 120, 1000, 131152):
        m = os.urandom(n)
        out = _buf(32)
        h.hs_sha256(out, m, C.c_size_t(n))
        assert out.raw == hashlib.sha256(m).digest()
        o.osha256(out, m, C.c_size_t(n))
        assert out.raw == hashlib.sha256(m).digest()
        h.hs_sha256_portable(out, m, C.c_size_t(n))   # the non-SHA-NI compression loop
        assert out.raw == hashlib.sha256(m).digest()
    # incremental updates with odd split points go through the same (SHA-NI or portable) block function
    assert h.hs_cpu_has_sha_ni() in (0, 1)


def test_fast_fp12_routines_match_the_generic_product(libs):
    """complex squaring, sparse line multiplication and cyclotomic squaring of the verification
    pairing (host_pairing.hpp) against the plain Karatsuba product"""
    o, h = libs
    for seed in range(40):
        assert h.hs_fp12_selftest(C.c_uint32(seed)) == 0, seed


# ---- 28-bit-limb device arithmetic (fp28.hpp, g1_28.hpp), host-compiled ----

def test_fp28_field_ops_match_oracle(libs):
    o, h = libs
    rnd = random.Random(9)
    edge = ac.FP_EDGES
    for k in range(400):
        a = edge[k % 7] if k < 49 else rnd.randrange(P)
        b = edge[(k // 7) % 7] if k < 49 else rnd.randrange(P)
        ab, bb = a.to_bytes(48, "little"), b.to_bytes(48, "little")
        r1, r2 = _buf(48), _buf(48)
        o.ofp_mul(r1, ab, bb)
        h.hs_fp28_mul(r2, ab, bb)
        assert r1.raw == r2.raw
        h.hs_fp28_roundtrip(r2, ab)
        assert r2.raw == ab
        o.ofp_sub(r1, ab, bb)
        h.hs_fp28_sub(r2, ab, bb)
        assert r1.raw == r2.raw
        o.ofp_add(r1, ab, ab)
        o.ofp_sub(r1, r1, bb)
        h.hs_fp28_addchain(r2, ab, bb)
        assert r1.raw == r2.raw


def test_fp28_conditional_negation_top_limb_edge(libs):
    # regression: a stored coordinate whose top 28-bit limb equals p's must negate correctly
    o, h = libs
    rnd = random.Random(1)
    r392, r384 = pow(2, 392, P), pow(2, 384, P)
    for k in range(600):
        if k < 400:
            t = ((P >> 364 << 364) - rnd.randrange(1 << 300) - 1) if k % 2 else (P - 1 - rnd.randrange(1 << 360))
            a = (t % P) * pow(r392, -1, P) % P
        else:
            a = rnd.randrange(P)
        b = rnd.randrange(P)
        am, bm = (a * r384 % P).to_bytes(48, "little"), (b * r384 % P).to_bytes(48, "little")
        for neg in (0, 1):
            r = _buf(48)
            h.hs_fp28_cneg_mul(r, am, bm, neg)
            assert int.from_bytes(r.raw, "little") == ((-a if neg else a) * b % P) * r384 % P


def test_xyzz28_mixed_addition_matches_oracle(libs):
    o, h = libs
    rnd = random.Random(11)
    g = _buf(144)
    h.hs_g1_generator(g)
    inf = _buf(144)
    for _ in range(8):
        p1, p2 = _omul(o, g, rnd.randrange(R)), _omul(o, g, rnd.randrange(R))
        a1, a2 = _buf(96), _buf(96)
        o.og1_to_affine(a1, p1)
        o.og1_to_affine(a2, p2)
        n2 = _buf(144)
        o.og1_neg(n2, p2)
        for neg, other in ((0, p2), (1, n2)):
            ref, r = _buf(144), _buf(144)
            o.og1_add(ref, p1, other)
            h.hs_g1_madd28(r, p1, a2, neg)
            assert o.og1_equal(r, ref)
        r = _buf(144)
        h.hs_g1_madd28(r, inf, a2, 1)           # accumulator at infinity, negated point
        assert o.og1_equal(r, n2)
        d, r = _buf(144), _buf(144)
        o.og1_dbl(d, p1)
        h.hs_g1_madd28(r, p1, a1, 0)            # same point: doubling path
        assert o.og1_equal(r, d)
        r = _buf(144)
        h.hs_g1_madd28(r, p1, a1, 1)            # P + (-P)
        assert o.og1_is_inf(r)
    n = 200
    pts, ref = _buf(96 * n), _buf(144)
    for i in range(n):
        p = _omul(o, g, rnd.randrange(R))
        a = _buf(96)
        o.og1_to_affine(a, p)
        pts[96 * i:96 * i + 96] = a.raw
        if i & 1:
            o.og1_neg(p, p)
        o.og1_add(ref, ref, p)
    r = _buf(144)
    h.hs_g1_madd28_chain(r, pts, n)
    assert o.og1_equal(r, ref)


def test_fp28_fused_two_product_reduction(libs):
    o, h = libs
    rnd = random.Random(19)
    edge = [0, 1, P - 1, P - 2, (P - 1) // 2, 2 ** 380]
    for k in range(400):
        v = [edge[(k // 6 ** i) % 6] for i in range(4)] if k < 200 else [rnd.randrange(P) for _ in range(4)]
        a, b, c, d = v
        bufs = [x.to_bytes(48, "little") for x in v]
        # operands are Montgomery residues on both sides: compare in that domain via the oracle
        t1, t2, t3, r1, r2 = _buf(48), _buf(48), _buf(48), _buf(48), _buf(48)
        o.ofp_sub(t1, bufs[1], bufs[2])
        o.ofp_mul(t1, bufs[0], t1)
        o.ofp_add(t1, t1, t1)            # 2a(b-c)
        o.ofp_mul(t2, bufs[2], bufs[3])  # c*d
        o.ofp_add(r1, t1, t2)
        h.hs_fp28_mul_add2(r2, bufs[0], bufs[1], bufs[2], bufs[3])
        assert r1.raw == r2.raw, k


def test_xyzz28_sign_alternating_accumulation(libs):
    """xyzz28_madd_alt keeps +-Y and flips the stored sign at every addition; chains with every
    special case in the middle (first point, doubling, cancellation to infinity, restart)."""
    o, h = libs
    rnd = random.Random(23)
    g = _buf(144)
    h.hs_g1_generator(g)

    def aff(p):
        a = _buf(96)
        o.og1_to_affine(a, p)
        return a.raw

    base = [_omul(o, g, rnd.randrange(R)) for _ in range(12)]
    scripts = ac.alternation_scripts(rnd)   # (index into base, subtract?) scripts
    for sc in scripts:
        special = None
        if isinstance(sc, tuple):
            special, sc = sc
        pts = b"".join(aff(base[i]) for i, _ in sc)
        signs = bytes(s for _, s in sc)
        ref = _buf(144)
        for i, sgn in sc:
            p = _buf(144)
            p.raw = base[i].raw
            if sgn:
                o.og1_neg(p, p)
            o.og1_add(ref, ref, p)
        if special == "dbl":
            # append the running sum itself as an affine point: forces the doubling path
            pts += aff(ref)
            signs += b"\x00"
            o.og1_dbl(ref, ref)
        r = _buf(144)
        h.hs_g1_madd28_alt_chain(r, pts, signs, len(signs))
        assert o.og1_equal(r, ref), sc


def test_fp28_square_and_inverse(libs):
    o, h = libs
    rnd = random.Random(13)
    edge = [1, 2, P - 1, P - 2, (P - 1) // 2, 2 ** 380]
    for k in range(300):
        a = edge[k % 6] if k < 36 else rnd.randrange(1, P)
        b = edge[(k // 6) % 6] if k < 36 else rnd.randrange(P)
        ab, bb = a.to_bytes(48, "little"), b.to_bytes(48, "little")
        r1, r2 = _buf(48), _buf(48)
        o.ofp_sqr(r1, ab)
        h.hs_fp28_sqr(r2, ab)
        assert r1.raw == r2.raw
        o.ofp_sub(r1, ab, bb)
        o.ofp_sqr(r1, r1)
        h.hs_fp28_sqr_lazy(r2, ab, bb)
        assert r1.raw == r2.raw
        if k < 40:
            o.ofp_inv(r1, ab)
            h.hs_fp28_inv(r2, ab)
            assert r1.raw == r2.raw


def test_xyzz28_full_add_mul_neg(libs):
    o, h = libs
    rnd = random.Random(17)
    g = _buf(144)
    h.hs_g1_generator(g)
    inf = _buf(144)
    for t in range(8):
        p1, p2 = _omul(o, g, rnd.randrange(R)), _omul(o, g, rnd.randrange(R))
        for a, b in ((p1, p2), (p1, p1), (inf, p2), (p1, inf)):
            ref, r = _buf(144), _buf(144)
            o.og1_add(ref, a, b)
            h.hs_g1_add28(r, a, b)
            assert o.og1_equal(r, ref)
        n1, r = _buf(144), _buf(144)
        o.og1_neg(n1, p1)
        h.hs_g1_add28(r, p1, n1)
        assert o.og1_is_inf(r)
        h.hs_g1_neg28(r, p1)
        assert o.og1_equal(r, n1)
        k = ac.W4_SCALARS[t] if t < 6 else rnd.randrange(R)
        kk = (C.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
        h.hs_g1_mul28(r, p1, kk)
        assert o.og1_equal(r, _omul(o, p1, k))
    # a point of order 3 (x = 0, y = 2): the windowed ladder must track infinities in its table
    r384 = pow(2, 384, P)
    pt = _buf(144)
    pt[48:96] = (2 * r384 % P).to_bytes(48, "little")
    pt[96:144] = (r384 % P).to_bytes(48, "little")
    for k in ac.ORDER3_SCALARS:
        kk = (C.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
        r = _buf(144)
        h.hs_g1_mul28(r, pt, kk)
        assert o.og1_equal(r, _omul(o, pt, k))


def test_jacobian_28bit_formulas(libs):
    """jac28_dbl / jac28_add (the coordinates of the scalar ladders) against the oracle, including
    the complete-addition special cases and long doubling chains (value-bound bookkeeping)."""
    o, h = libs
    rnd = random.Random(37)
    g = _buf(144)
    h.hs_g1_generator(g)
    inf = _buf(144)
    for t in range(10):
        p1, p2 = _omul(o, g, rnd.randrange(1, R)), _omul(o, g, rnd.randrange(1, R))
        named = {"p1": p1, "p2": p2, "inf": inf}
        for a, b, neg in ((named[x], named[y], sg) for x, y, sg in ac.JAC_ADD_TUPLES):
            ref, r, bb = _buf(144), _buf(144), _buf(144)
            bb.raw = b.raw
            if neg:
                o.og1_neg(bb, bb)
            o.og1_add(ref, a, bb)
            h.hs_g1_jac28_add(r, a, b, neg)
            assert o.og1_equal(r, ref), (t, neg)
        n = ac.DBL_CHAIN_LENGTHS[t % 6]
        ref, r = _buf(144), _buf(144)
        ref.raw = p1.raw
        for _ in range(n):
            o.og1_dbl(ref, ref)
        h.hs_g1_jac28_dbl_chain(r, p1, n)
        assert o.og1_equal(r, ref), n


def test_glv_split_and_glv_scalar_mul(libs):
    """k = k1 + k2*lambda with both halves < 2^128 (lambda = x^2 - 1), and the two-dimensional
    ladder [k1]P + [k2]phi(P) of the G1 FFT equals [k]P for subgroup points."""
    o, h = libs
    rnd = random.Random(29)
    lam = LAMBDA
    assert (lam * lam + lam + 1) == R
    g = _buf(144)
    h.hs_g1_generator(g)
    ks = ac.glv_scalars(rnd)
    p1 = _omul(o, g, rnd.randrange(1, R))
    for n, k in enumerate(ks):
        kk = (C.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
        out = (C.c_uint32 * 8)()
        h.hs_glv_split(out, kk)
        k1 = sum(out[i] << (32 * i) for i in range(4))
        k2 = sum(out[4 + i] << (32 * i) for i in range(4))
        assert k1 == k % lam and k2 == k // lam and k1 + k2 * lam == k
        if n < 30:
            r = _buf(144)
            h.hs_g1_mul28_glv(r, p1, kk)
            assert o.og1_equal(r, _omul(o, p1, k)), k
            h.hs_g1_mul_glv_host(r, p1, kk)      # joint double-and-add of the host verification path
            assert o.og1_equal(r, _omul(o, p1, k)), k
            h.hs_g1_mul28_glv_naf(r, p1, kk)     # width-4 NAF ladder of the G1 FFT twiddles
            assert o.og1_equal(r, _omul(o, p1, k)), k
        naf = (C.c_int8 * 132)()
        h.hs_wnaf4_128(naf, (C.c_uint32 * 4)(*[(k1 >> (32 * i)) & 0xffffffff for i in range(4)]))
        assert sum(int(naf[i]) << i for i in range(132)) == k1
        assert all(d == 0 or (d % 2 and abs(d) <= 7) for d in naf)
        assert all(sum(1 for d in naf[i:i + 4] if d) <= 1 for i in range(129))
    r = _buf(144)
    kk = (C.c_uint32 * 8)(*[(ks[20] >> (32 * i)) & 0xffffffff for i in range(8)])
    h.hs_g1_mul28_glv(r, _buf(144), kk)   # infinity in, infinity out
    assert o.og1_is_inf(r)


def test_generator_table_and_split_miller_loops(libs):
    """host_pairing.hpp: [k]G1 from the 64 x 15 generator table against the generic ladder, and the product check
    with the second pair's Miller loop run ahead of time against the fused loop (true and false instances)."""
    o, h = libs
    rnd = random.Random(91)
    ks = [0, 1, 15, 16, 17, R - 1, R - 2, 2 ** 252, (1 << 255) % R, 0x0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f]
    ks += [rnd.randrange(R) for _ in range(30)]
    for k in ks:
        kk = (C.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
        assert h.hs_g1_gen_mul_check(kk) == 1, k
    g, g2 = _buf(144), _buf(288)
    h.hs_g1_generator(g)
    h.hs_g2_generator(g2)
    k = rnd.randrange(1, R)
    kk = (C.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
    kg2 = _buf(288)
    h.hs_g2_mul(kg2, g2, kk, 255)
    kg1 = _omul(o, g, k)
    neg_g = _omul(o, g, R - 1)
    # e(kG, Q) * e(-G, kQ) == 1 ; e(kG, Q) * e(G, kQ) != 1
    assert h.hs_pairing_split(kg1, g2, neg_g, kg2) == 3
    assert h.hs_pairing_split(kg1, g2, g, kg2) == 2
    # an infinite argument on either side
    inf = _buf(144)
    assert h.hs_pairing_split(inf, g2, inf, kg2) == 3
    assert h.hs_pairing_split(kg1, g2, inf, kg2) == 2


def test_coz_table_and_mixed_addition_branches(libs):
    """g1_28.hpp: the co-Z table {P, 3P, 5P, 7P} of the G1 FFT's NAF ladder brought home from its isomorphic curve,
    and every branch of the mixed addition on that curve (from infinity, equal points -> doubling, generic,
    opposite points -> infinity, the phi image of an entry)."""
    o, h = libs
    rnd = random.Random(77)
    lam = (0xd201000000010000 ** 2 - 1)
    g = _buf(144)
    h.hs_g1_generator(g)
    for _ in range(6):
        p1 = _omul(o, g, rnd.randrange(1, R))
        out = _buf(9 * 144)
        h.hs_je28_cases(out, p1)
        got = [C.create_string_buffer(out.raw[144 * i:144 * (i + 1)], 144) for i in range(9)]
        for m in range(4):
            assert o.og1_equal(got[m], _omul(o, p1, 2 * m + 1)), m
        assert o.og1_equal(got[4], p1)
        assert o.og1_equal(got[5], _omul(o, p1, 2))
        assert o.og1_equal(got[6], _omul(o, p1, 5))
        assert o.og1_is_inf(got[7])
        assert o.og1_equal(got[8], _omul(o, p1, (2 + 7 * lam) % R))


def test_fr_safegcd_inverse(libs):
    """fr_inv.hpp (the inversion of the barycentric evaluation kernel) against Python and the Fermat ladder"""
    o, h = libs
    rnd = random.Random(41)
    r256 = pow(2, 256, R)
    vals = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, 3, 7, 2 ** 254, 2 ** 255 - 19 - R, R - 3, 2 ** 32, 2 ** 32 - 1]
    vals += [rnd.randrange(R) for _ in range(3000)]
    for a in vals:
        ab = (a * r256 % R).to_bytes(32, "little")
        r1, r2 = _buf(32), _buf(32)
        h.hs_fr_inv_safegcd(r1, ab)
        got = int.from_bytes(r1.raw, "little") * pow(r256, -1, R) % R
        assert got == (pow(a, -1, R) if a else 0), a
        if a < 2 ** 33 or a > R - 4:
            h.hs_fr_inv_fermat(r2, ab)
            assert r1.raw == r2.raw


def test_endomorphism_subgroup_test_is_exact(libs):
    """g1_28_in_subgroup ([x^2]P == (beta^2 X, -Y)) against the oracle's [r]P == inf on points of
    G1, of the cofactor subgroup, mixed points, the order-3 point and random curve points."""
    o, h = libs
    rnd = random.Random(31)
    r384 = pow(2, 384, P)

    def curve_point(x0):
        x, y = ac.curve_point_xy(x0)
        pt = _buf(144)
        pt[0:48] = (x * r384 % P).to_bytes(48, "little")
        pt[48:96] = (y * r384 % P).to_bytes(48, "little")
        pt[96:144] = (r384 % P).to_bytes(48, "little")
        return pt

    def check(pt, expect=None):
        a = _buf(96)
        o.og1_to_affine(a, pt)
        want = bool(o.og1_in_subgroup(pt))
        if expect is not None:
            assert want == expect
        assert h.hs_g1_in_subgroup28(a) == (1 if want else 0)
        assert h.hs_g1_in_subgroup_host(a) == (1 if want else 0)   # same test on the host's Jacobian code

    o.og1_in_subgroup.restype = C.c_bool
    g = _buf(144)
    h.hs_g1_generator(g)
    rk = (C.c_uint64 * 4)(*[(R >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])
    for t in range(6):
        check(_omul(o, g, rnd.randrange(1, R)), True)
    check(curve_point(0), False)                      # (0, 2): order 3
    for t in range(6):
        pt = curve_point(rnd.randrange(P))
        check(pt, False)                              # a random curve point is outside G1
        tors = _buf(144)
        o.og1_mul_raw(tors, pt, rk, 255)              # [r]P: in the cofactor subgroup, not in G1
        assert not o.og1_is_inf(tors)
        check(tors, False)
        mixed = _buf(144)
        o.og1_add(mixed, tors, _omul(o, g, rnd.randrange(1, R)))
        check(mixed, False)


def test_safegcd_inverse_matches_fermat_and_python(libs):
    o, h = libs
    rnd = random.Random(19)
    r384 = pow(2, 384, P)
    vals = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, 3, 7, 2 ** 380, 2 ** 381 - 1, P - 3]
    vals += [rnd.randrange(P) for _ in range(1500)]
    for a in vals:
        ab = (a * r384 % P).to_bytes(48, "little")
        r1, r2 = _buf(48), _buf(48)
        h.hs_fp28_inv_safegcd(r1, ab)
        got = int.from_bytes(r1.raw, "little") * pow(r384, -1, P) % P
        assert got == (pow(a, -1, P) if a else 0)
        if a < 2 ** 20 or a > P - 4:
            h.hs_fp28_inv(r2, ab)  # sliding-window Fermat ladder
            assert r1.raw == r2.raw


def test_glv_split_signed_and_window_recoding(libs):
    """glv_split_signed / recode_signed_128 (g1_28.hpp) feed every fixed-base MSM kernel: k must equal
    s1*m1 + lambda*s2*m2 mod r with both magnitudes small enough that no table width carries out of its
    top window, and the signed digits must rebuild the half-scalar and stay inside the table."""
    _, h = libs
    assert (LAMBDA * LAMBDA + LAMBDA + 1) == R
    rnd = random.Random(99)
    edge = [0, 1, 2, R - 1, R - 2, LAMBDA, LAMBDA - 1, LAMBDA + 1, LAMBDA // 2, LAMBDA // 2 + 1,
            (LAMBDA + 1) * (LAMBDA // 2), (LAMBDA + 1) * (LAMBDA // 2) + LAMBDA // 2 + 1, R // 2, R // 3,
            LAMBDA * LAMBDA, LAMBDA * LAMBDA + LAMBDA, (1 << 254), (1 << 128) - 1, (1 << 128), (1 << 127)]
    edge += [q * LAMBDA + t for q in (1, 2, LAMBDA // 2, LAMBDA // 2 + 1, LAMBDA - 1, LAMBDA)
             for t in (0, 1, LAMBDA // 2, LAMBDA // 2 + 1, LAMBDA - 1) if q * LAMBDA + t < R]
    bound = (LAMBDA + 3) // 2
    for it in range(20000):
        k = edge[it] if it < len(edge) else rnd.randrange(R)
        kk = (C.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
        m1, m2 = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
        n1, n2 = C.c_int(), C.c_int()
        h.hs_glv_split_signed(kk, m1, C.byref(n1), m2, C.byref(n2))
        a = sum(v << (32 * i) for i, v in enumerate(m1))
        b = sum(v << (32 * i) for i, v in enumerate(m2))
        assert a <= bound and b <= bound, (k, a, b)
        sa, sb = (-a if n1.value else a), (-b if n2.value else b)
        assert (sa + LAMBDA * sb - k) % R == 0, k
        if it % 7 == 0 or it < len(edge):
            for wbits in (4, 7, 8, 10, 13, 15, 16):
                nwh = 127 // wbits + 1
                for m, neg, sv in ((m1, n1.value, sa), (m2, n2.value, sb)):
                    dg = (C.c_int16 * nwh)()
                    h.hs_recode_signed_128(dg, m, neg, wbits, nwh)
                    assert sum(int(d) << (wbits * w) for w, d in enumerate(dg)) == sv, (k, wbits)
                    assert all(abs(int(d)) <= (1 << (wbits - 1)) for d in dg)


def test_fixed_base_glv_msm_algorithm_matches_oracle(libs):
    """The accumulate kernels' algorithm (GLV digits -> half-width table entries -> sign-alternating mixed
    additions -> phi once per lane -> fold), replayed on the host with the same inline functions
    (hs_msm_glv_emulate), equals sum k_i P_i computed by the oracle -- for several table widths, lane
    counts that do and do not split at the half boundary, and scalars that exercise every centring case."""
    o, h = libs
    rnd = random.Random(2027)
    g = _buf(144)
    h.hs_g1_generator(g)
    n = 6
    pts_j = [_omul(o, g, rnd.randrange(1, R)) for _ in range(n)]
    aff = _buf(96 * n)
    for i, p in enumerate(pts_j):
        a = _buf(96)
        o.og1_to_affine(a, p)
        aff[96 * i:96 * (i + 1)] = a.raw
    special = [0, 1, R - 1, LAMBDA, LAMBDA + 1, LAMBDA // 2 + 1, (LAMBDA + 1) * (LAMBDA // 2 + 1)]
    for wbits, lanes in ((4, 1), (5, 7), (8, 64), (13, 16), (16, 3)):
        ks = [special[(i + wbits) % len(special)] if i < 3 else rnd.randrange(R) for i in range(n)]
        sc = (C.c_uint32 * (8 * n))(*[(k >> (32 * j)) & 0xffffffff for k in ks for j in range(8)])
        got = _buf(144)
        h.hs_msm_glv_emulate(got, aff, sc, n, wbits, lanes)
        acc = None
        for p, k in zip(pts_j, ks):
            t = _omul(o, p, k)
            if acc is None:
                acc = t
            else:
                s = _buf(144)
                o.og1_add(s, acc, t)
                acc = s
        assert o.og1_equal(got, acc), (wbits, lanes)


def _brp(i, bits):
    return int(bin(i)[2:].zfill(bits)[::-1], 2)


def test_fr29_arithmetic(libs):
    """fr29.hpp (Fr on nine 29-bit limbs, radix 2^261: the arithmetic of k_eval_barycentric) against Python integers:
    products, the mixed-radix product, the canonical subtraction, the lazy sums and the inversion."""
    o, h = libs
    rnd = random.Random(2929)
    r256 = pow(2, 256, R)
    mont = lambda v: (v * r256 % R).to_bytes(32, "little")
    unm = lambda b: int.from_bytes(b.raw, "little") * pow(r256, -1, R) % R
    edge = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, 2 ** 254, 2 ** 32, 2 ** 29 - 1, 2 ** 29, R - 2 ** 29, 2 ** 232, 2 ** 232 - 1]
    vals = edge + [rnd.randrange(R) for _ in range(400)]
    for k, a in enumerate(vals):
        b = vals[(7 * k + 3) % len(vals)]
        out = _buf(32)
        h.hs_fr29_roundtrip(out, mont(a))
        assert out.raw == mont(a)
        h.hs_fr29_mul(out, mont(a), mont(b))
        assert out.raw == mont(a * b % R), (a, b)
        h.hs_fr29_mul_mixed(out, mont(a), mont(b))
        assert out.raw == mont(a * b % R), (a, b)
        h.hs_fr29_sub(out, mont(a), mont(b))
        assert out.raw == mont((a - b) % R), (a, b)
        if a:
            h.hs_fr29_inv(out, mont(a))
            assert unm(out) == pow(a, -1, R), a
    for n in (1, 2, 3, 4, 5, 8, 15, 16, 17, 32):
        for worst in (False, True):
            xs = [R - 1 - i if worst else rnd.randrange(R) for i in range(n)]
            out = _buf(32)
            h.hs_fr29_sum(out, b"".join(x.to_bytes(32, "little") for x in xs), n)
            assert int.from_bytes(out.raw, "little") == sum(xs) % R, (n, worst)


def test_fr29_barycentric_evaluation(libs):
    """the kernel's algorithm replayed thread by thread on the host (prefix products per thread, one inversion per
    lane of the first wave for four waves' products, terms that come out in the library's radix) against
    evaluate_polynomial_in_evaluation_form (src/eip4844/eip4844.c:192-240) computed with Python integers;
    z inside the domain (eip4844.c:208-215), polynomials of extreme values, and the parked inverses."""
    o, h = libs
    rnd = random.Random(61)
    r256 = pow(2, 256, R)
    w = pow(7, (R - 1) // 4096, R)
    roots = [pow(w, _brp(i, 12), R) for i in range(4096)]
    roots_b = b"".join((x * r256 % R).to_bytes(32, "little") for x in roots)
    n_inv = pow(4096, -1, R)

    def ref(poly, z):
        if z in roots:
            return poly[roots.index(z)]
        s = sum(p * x % R * pow((z - x) % R, -1, R) for p, x in zip(poly, roots)) % R
        return s * (pow(z, 4096, R) - 1) % R * n_inv % R

    cases = []
    cases.append(([rnd.randrange(R) for _ in range(4096)], rnd.randrange(R)))
    cases.append(([R - 1] * 4096, R - 1))
    cases.append(([0] * 4096, 5))
    cases.append(([rnd.randrange(R) for _ in range(4096)], 0))
    cases.append(([rnd.randrange(R) for _ in range(4096)], roots[1234]))
    cases.append(([rnd.randrange(R) for _ in range(4096)], roots[0]))
    cases.append(([rnd.randrange(R) for _ in range(4096)], (roots[4095] + 1) % R))
    for poly, z in cases:
        pb = b"".join((p * r256 % R).to_bytes(32, "little") for p in poly)
        y = _buf(32)
        di = _buf(4096 * 32)
        hit = h.hs_fr29_eval(y, di, pb, (z * r256 % R).to_bytes(32, "little"), roots_b)
        assert int.from_bytes(y.raw, "little") == ref(poly, z) * r256 % R
        # the inversion-free tree (k_eval_tree): one wave per polynomial and four
        for log_per in (6, 4):
            y2 = _buf(32)
            h.hs_fr29_eval_tree(y2, pb, (z * r256 % R).to_bytes(32, "little"), roots_b, log_per)
            assert y2.raw == y.raw, log_per
            # the same tree over the blob's bytes (conversion and range check folded in)
            y3 = _buf(32)
            bad = (C.c_uint32 * 1)(0)
            blob = b"".join(p.to_bytes(32, "big") for p in poly)
            h.hs_fr29_eval_tree_bytes(y3, bad, blob, (z * r256 % R).to_bytes(32, "little"), roots_b, log_per)
            assert y3.raw == y.raw and bad[0] == 0, log_per
        assert hit == (roots.index(z) if z in roots else -1)
        if hit < 0:
            r261 = pow(2, 261, R)
            for i in (0, 1, 255, 256, 2047, 4095):
                got = int.from_bytes(di.raw[32 * i:32 * i + 32], "little")
                assert got == pow((z - roots[i]) % R, -1, R) * r261 % R, i


def test_fr29_tree_over_bytes_flags_non_canonical_elements(libs):
    """k_eval_tree's BYTES form: an element >= r anywhere in the blob sets the flag (bytes_to_bls_field,
    src/common/bytes.c:52-70); r - 1 does not."""
    o, h = libs
    r256 = pow(2, 256, R)
    w = pow(7, (R - 1) // 4096, R)
    roots_b = b"".join((pow(w, _brp(i, 12), R) * r256 % R).to_bytes(32, "little") for i in range(4096))
    z = (12345 * r256 % R).to_bytes(32, "little")
    for pos in (0, 1, 63, 64, 2047, 4095):
        for val, want in ((R - 1, 0), (R, 1), (R + 1, 1), (2 ** 256 - 1, 1), (R + 2 ** 232, 1)):
            elems = [7] * 4096
            elems[pos] = val
            blob = b"".join(e.to_bytes(32, "big") for e in elems)
            for log_per in (6, 4):
                y = _buf(32)
                bad = (C.c_uint32 * 1)(0)
                h.hs_fr29_eval_tree_bytes(y, bad, blob, z, roots_b, log_per)
                assert bad[0] == want, (pos, hex(val), log_per)
