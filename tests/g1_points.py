"""An independent model of G1 for the validation tests: plain Python integers, no oracle, no library.

The curve is E: y^2 = x^3 + 4 over Fp.  #E(Fp) = h * r with the cofactor h = 3 * 11^2 * 10177^2 * 859267^2 * 52437899^2;
G1 is the subgroup of order r.  Membership is decided by its definition, [r]P == infinity -- not by the endomorphism
identity the product uses.  Encodings follow the ZCash compressed form that src/common/bytes.c:81-95 accepts (through
blst_p1_uncompress): flag bits 0x80 (compressed, required), 0x40 (infinity: every other bit zero), 0x20 (y is the
lexicographically larger root), then x big-endian, x < p.

corpus() returns Entry(label, data, expected, point) with expected one of VALID / NOT_IN_G1 / BAD_ENCODING; point is
the affine (x, y) of a curve point, INF for infinity, None for a bad encoding."""
import collections
import random

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
TORSION_PRIMES = (11, 10177, 859267, 52437899)
H = 3 * 11 ** 2 * 10177 ** 2 * 859267 ** 2 * 52437899 ** 2
# the generator (draft-irtf-cfrg-pairing-friendly-curves, BLS12-381 G1)
GX = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
GY = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1
assert H == 0x396c8c005555e1568c00aaab0000aaab   # the published cofactor of G1

VALID, NOT_IN_G1, BAD_ENCODING = "valid", "not_in_g1", "bad_encoding"
Entry = collections.namedtuple("Entry", "label data expected point")

INF = "infinity"   # the point at infinity (affine); compared with `is`


# ---- Fp and the curve (Jacobian: X/Z^2, Y/Z^3; Z == 0 is infinity) ----

def on_curve(pt):
    x, y = pt
    return (y * y - x * x * x - 4) % P == 0


def sqrt_fp(a):
    """a square root of a (p = 3 mod 4), or None"""
    y = pow(a % P, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def _jac(pt):
    return (0, 1, 0) if pt is INF else (pt[0], pt[1], 1)


def _aff(j):
    x, y, z = j
    if z % P == 0:
        return INF
    zi = pow(z, -1, P)
    zi2 = zi * zi % P
    return (x * zi2 % P, y * zi2 * zi % P)


def _dbl(j):
    x, y, z = j
    if z == 0 or y == 0:
        return (0, 1, 0)
    a = x * x % P
    b = y * y % P
    c = b * b % P
    d = 2 * ((x + b) * (x + b) - a - c) % P
    e = 3 * a % P
    x3 = (e * e - 2 * d) % P
    return (x3, (e * (d - x3) - 8 * c) % P, 2 * y * z % P)


def _add(j1, j2):
    x1, y1, z1 = j1
    x2, y2, z2 = j2
    if z1 == 0:
        return j2
    if z2 == 0:
        return j1
    z1z1, z2z2 = z1 * z1 % P, z2 * z2 % P
    u1, u2 = x1 * z2z2 % P, x2 * z1z1 % P
    s1, s2 = y1 * z2 * z2z2 % P, y2 * z1 * z1z1 % P
    if u1 == u2:
        return _dbl(j1) if s1 == s2 else (0, 1, 0)
    hh = (u2 - u1) % P
    i = 4 * hh * hh % P
    jj = hh * i % P
    rr = 2 * (s2 - s1) % P
    v = u1 * i % P
    x3 = (rr * rr - jj - 2 * v) % P
    y3 = (rr * (v - x3) - 2 * s1 * jj) % P
    z3 = ((z1 + z2) * (z1 + z2) - z1z1 - z2z2) * hh % P
    return (x3, y3, z3)


def add(a, b):
    return _aff(_add(_jac(a), _jac(b)))


def neg(a):
    return INF if a is INF else (a[0], (-a[1]) % P)


def mul(a, k):
    """[k]a for k >= 0"""
    acc, base = (0, 1, 0), _jac(a)
    for bit in bin(k)[2:] if k else "":
        acc = _dbl(acc)
        if bit == "1":
            acc = _add(acc, base)
    return _aff(acc)


def in_g1(a):
    """membership by definition: [r]P == infinity"""
    return a is INF or mul(a, R) is INF


G = (GX, GY)
assert on_curve(G) and in_g1(G)


# ---- encodings ----

def compress(a):
    if a is INF:
        return bytes([0xc0]) + bytes(47)
    x, y = a
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if y > (P - 1) // 2 else 0)
    return bytes(b)


def uncompress(data):
    """(status, point): status 0 ok (point may be INF), 1 bad encoding, 2 not on the curve"""
    b0 = data[0]
    if not b0 & 0x80:
        return 1, None
    if b0 & 0x40:
        if b0 & 0x3f or any(data[1:]):
            return 1, None
        return 0, INF
    x = int.from_bytes(bytes([b0 & 0x1f]) + data[1:], "big")
    if x >= P:
        return 1, None
    y = sqrt_fp(x * x * x + 4)
    if y is None:
        return 2, None
    if (y > (P - 1) // 2) != bool(b0 & 0x20):
        y = P - y
    return 0, (x, y)


def classify(data):
    """what bytes_to_kzg_commitment makes of 48 bytes"""
    st, pt = uncompress(data)
    if st:
        return BAD_ENCODING
    return VALID if in_g1(pt) else NOT_IN_G1


def _raw_x(x, flags=0x80):
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


# ---- points outside G1 ----

def curve_point_at(x):
    """the first curve point with abscissa >= x (the smaller root of y)"""
    while True:
        y = sqrt_fp(x * x * x + 4)
        if y is not None:
            return (x, min(y, P - y))
        x += 1


def torsion_point(ell, rnd):
    """a point of order exactly ell (ell^2 divides h: the ell-part of E(Fp) is Z/ell x Z/ell, killed by h r / ell)"""
    assert H % (ell * ell) == 0 and H % (ell ** 3) != 0
    while True:
        t = mul(curve_point_at(rnd.randrange(P)), H * R // (ell * ell))
        if t is not INF:
            assert mul(t, ell) is INF
            return t


T3 = (0, 2)
assert on_curve(T3) and mul(T3, 3) is INF


def _build():
    rnd = random.Random(0x61C0)
    out = []

    def put(label, pt, expected):
        out.append(Entry(label, compress(pt), expected, pt))

    # valid
    put("G", G, VALID)
    put("-G", neg(G), VALID)
    for i in range(2):
        put("kG%d" % i, mul(G, rnd.randrange(2, R - 1)), VALID)
    put("(r-1)G", mul(G, R - 1), VALID)
    put("inf", INF, VALID)
    q = mul(G, rnd.randrange(2, R - 1))
    put("Q", q, VALID)
    put("-Q", neg(q), VALID)   # the same x, the sign bit flipped
    assert compress(q)[1:] == compress(neg(q))[1:] and compress(q)[0] ^ compress(neg(q))[0] == 0x20

    # outside G1, each with its negation
    bad = [("T3", T3)]
    for ell in TORSION_PRIMES:
        for k in range(2):
            bad.append(("T%d_%d" % (ell, k), torsion_point(ell, rnd)))
    for ell in TORSION_PRIMES:
        bad.append(("Q+T%d" % ell, add(q, torsion_point(ell, rnd))))
    bad.append(("generic", curve_point_at(1)))
    for label, pt in bad:
        put(label, pt, NOT_IN_G1)
        put("neg(%s)" % label, neg(pt), NOT_IN_G1)

    # bad encodings
    g = compress(G)
    out.append(Entry("no_compression_bit", bytes([g[0] & 0x7f]) + g[1:], BAD_ENCODING, None))
    out.append(Entry("inf_with_x", bytes([0xc0]) + bytes(46) + b"\x01", BAD_ENCODING, None))
    out.append(Entry("inf_with_sign", bytes([0xe0]) + bytes(47), BAD_ENCODING, None))
    out.append(Entry("x=p", _raw_x(P), BAD_ENCODING, None))
    out.append(Entry("x=p+1", _raw_x(P + 1), BAD_ENCODING, None))
    out.append(Entry("x=2^381-1", _raw_x(2 ** 381 - 1), BAD_ENCODING, None))
    x = 1
    while sqrt_fp(x ** 3 + 4) is not None:
        x += 1
    out.append(Entry("off_curve", _raw_x(x), BAD_ENCODING, None))
    out.append(Entry("off_curve_sign", _raw_x(x, 0xa0), BAD_ENCODING, None))
    return out


_CORPUS = None


def corpus():
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = _build()
    return list(_CORPUS)


def by_label(label):
    return next(e for e in corpus() if e.label == label)
