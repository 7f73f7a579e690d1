"""ckzg_hip_g1_fft (c-kzg-4844_amd/csrc/g1_fft.hip, g1_fft_plan.hpp): the G1 transform at every power of two up to 8192
on points a G with known a.  Expected scalars come from a Python-integer transform (tests/domain_expect.py); outputs are
compared as points through the oracle (its additions over a table of multiples of G)."""
import ctypes as C
import random

import pytest

import domain_expect as D
import g1_points as GP
from conftest import ORACLE_SO
from test_gpu_locate import G1

pytestmark = pytest.mark.gpu
R = D.R
BADARGS = 1
QUAD_MAX = 8192   # g1_fft_plan.hpp: G1_FFT_QUAD_MAX_DEFAULT (tests/test_domain_openings_cpu.py pins it and the picker)


class GenTable:
    """[e]G for a known e through the oracle: 32 additions from a table of d 256^w G"""

    def __init__(self, g1):
        self.g1, self.rows = g1, []
        base = g1.gen
        for _ in range(32):
            row, acc = [g1.inf], g1.inf
            for _ in range(255):
                acc = g1.add(acc, base)
                row.append(acc)
            self.rows.append(row)
            base = g1.add(acc, base)   # 256 * base

    def mul(self, e):
        acc = self.g1.inf
        for w in range(32):
            d = (e >> (8 * w)) & 255
            if d:
                acc = self.g1.add(acc, self.rows[w][d])
        return acc


@pytest.fixture(scope="module")
def g1():
    return G1()


@pytest.fixture(scope="module")
def gen(g1):
    t = GenTable(g1)
    k = random.Random(1).randrange(R)
    assert g1.eq(t.mul(k), g1.mul(g1.gen, k)) and g1.eq(t.mul(R - 1), g1.neg(g1.gen))
    return t


@pytest.fixture(scope="module")
def pool(g1, gen):
    """200 points a G with known a and a Z that is not one (the oracle's addition of two multiples)"""
    rnd = random.Random(12)
    out = []
    for _ in range(200):
        a, j = rnd.randrange(1, R), rnd.randrange(1, R)
        out.append((a, g1.add(gen.mul((a - j) % R), gen.mul(j))))
    return out


def _expected(scalars, n, inverse):
    if n == 1:
        return list(scalars)
    w = D.root_of_unity(n)
    out = []
    for f in range(len(scalars) // n):
        out += D.fft(scalars[f * n:(f + 1) * n], pow(w, -1, R) if inverse else w)
    return out


def _check(hip, g1, gen, scalars, points, n, inverse, idx=None):
    out = hip.g1_fft(points, n, inverse)
    assert len(out) == len(points)
    exp = _expected(scalars, n, inverse)
    for i in (range(len(out)) if idx is None else idx):
        assert g1.eq(out[i], gen.mul(exp[i])), (n, inverse, i)
    return out


def _random_input(pool, total, seed):
    rnd = random.Random(seed)
    picks = [pool[rnd.randrange(len(pool))] for _ in range(total)]
    return [a for a, _ in picks], [p for _, p in picks]


# n <= 128 with 1, 3 and 65 transforms, 256 alone: every output.  All of these are the four-lane form (at most 65 * 63
# ladders in a launch).
SMALL = [(n, c) for n in (1, 2, 4, 8, 64, 128) for c in (1, 3, 65)] + [(256, 1)]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n,count", SMALL)
def test_every_output_small(hip, g1, gen, pool, n, count, inverse):
    scalars, points = _random_input(pool, n * count, 1000 * n + count)
    if n * count >= 4:   # the identity among the inputs, and a repeated point
        scalars[1], points[1] = 0, g1.inf
        scalars[3], points[3] = scalars[2], points[2]
    _check(hip, g1, gen, scalars, points, n, inverse)


# The hand-over between the forms at n = 128 (63 ladders per transform in the last stage): 130 transforms are 8190
# products, the four-lane form; 131 are 8253, one lane per half-product.  Every output.
@pytest.mark.parametrize("count,inverse", [(130, False), (131, True)])
def test_every_output_at_the_hand_over(hip, g1, gen, pool, count, inverse):
    assert 63 * 130 <= QUAD_MAX < 63 * 131
    scalars, points = _random_input(pool, 128 * count, count)
    _check(hip, g1, gen, scalars, points, 128, inverse)


# 4096 and 8192: outputs 0, 1, n/2, n-1 and 256 seeded indices of every transform exactly, and inverse(forward(x)) =
# [n] x for every entry.  (8192, 2) is the last size of the four-lane form, (8192, 3) the first of the one-lane form;
# in the early stages of (8192, 3) a wave holds 64 different twiddles.
@pytest.mark.parametrize("n,count", [(4096, 1), (8192, 1), (8192, 2), (8192, 3)])
def test_large(hip, g1, gen, pool, n, count):
    assert (count * (n // 2 - 1) <= QUAD_MAX) == ((n, count) != (8192, 3))
    scalars, points = _random_input(pool, n * count, n + count)
    scalars[5], points[5] = 0, g1.inf
    rnd = random.Random(n * count)
    idx = sorted({f * n + i for f in range(count) for i in [0, 1, n // 2, n - 1] + [rnd.randrange(n) for _ in range(256)]})
    fwd = _check(hip, g1, gen, scalars, points, n, False, idx)
    _check(hip, g1, gen, scalars, points, n, True, idx)
    back = hip.g1_fft(fwd, n, True)
    scaled = {}
    for i, p in enumerate(points):
        if p not in scaled:
            r = C.create_string_buffer(144)
            g1.o.og1_mul_raw(r, p, (C.c_uint64 * 4)(n, 0, 0, 0), 14)
            scaled[p] = r.raw
        assert g1.eq(back[i], scaled[p]), i


@pytest.mark.parametrize("n", [2, 8, 128, 4096, 8192])
def test_chosen_inputs(hip, g1, gen, pool, n):
    a, p = pool[7]
    w = D.root_of_unity(n)
    some = sorted({0, 1, n // 2, n - 1} | ({random.Random(n).randrange(n) for _ in range(64)} if n > 256 else set(range(n))))
    # all entries equal to P: every first butterfly doubles, every u - v is the identity; out = [n P, 0, 0, ...]
    out = hip.g1_fft([p] * n, n)
    assert g1.eq(out[0], gen.mul(n * a % R)) and all(g1.eq(out[i], g1.inf) for i in range(1, n))
    # the delta at index 0: every output is P
    out = hip.g1_fft([p] + [g1.inf] * (n - 1), n)
    assert all(g1.eq(out[i], p) for i in some)
    # the delta at index 1: out[k] = [w^k] P, every twiddle exactly (all of them up to 256, 68 of them above)
    for inverse in (False, True):
        out = hip.g1_fft([g1.inf, p] + [g1.inf] * (n - 2), n, inverse)
        for k in some:
            assert g1.eq(out[k], gen.mul(a * pow(w, -k if inverse else k, R) % R)), (n, inverse, k)
    # P, -P pairs: u + v is the identity in every first butterfly of the DIF pass (span n/2) when n >= 4 ...
    pts = [p if (i // max(n // 2, 1)) % 2 == 0 else g1.neg(p) for i in range(n)]
    sc = [a if (i // max(n // 2, 1)) % 2 == 0 else R - a for i in range(n)]
    _check(hip, g1, gen, sc, pts, n, False, some)
    # ... and alternating P, -P: out[n/2] = [n] P, the rest the identity
    out = hip.g1_fft([p if i % 2 == 0 else g1.neg(p) for i in range(n)], n)
    assert all(g1.eq(out[i], gen.mul(n * a % R) if i == n // 2 else g1.inf) for i in some)
    # all identity
    out = hip.g1_fft([g1.inf] * n, n, True)
    assert all(g1.eq(q, g1.inf) for q in out)


def test_empty_and_copy(hip, g1, pool):
    assert hip.g1_fft([], 0) == [] and hip.g1_fft([], 8) == []
    pts = [pool[i][1] for i in range(5)]
    out = hip.g1_fft(pts, 1)
    assert all(g1.eq(a, b) for a, b in zip(out, pts))


# ---- rejections: C_KZG_BADARGS and `out` untouched ----

def _mont(x):
    return (x * pow(2, 384, GP.P) % GP.P).to_bytes(48, "little")


def _g1_t(pt):
    """an affine point (x, y) as a g1_t with Z = 1"""
    return _mont(pt[0]) + _mont(pt[1]) + _mont(1)


def _raw_call(hip, points, n, count, inverse=0):
    size = 144 * max(len(points), 1)
    out = C.create_string_buffer(b"\xa5" * size, size)
    f = hip.lib.ckzg_hip_g1_fft
    f.restype = C.c_int
    ret = f(out, b"".join(points), C.c_uint64(n), C.c_uint64(count), C.c_int(inverse), hip.sp)
    return ret, out.raw == b"\xa5" * size


def test_rejections(hip, g1, pool):
    pts = [pool[i % 200][1] for i in range(16)]
    # the helper builds what the library reads: a good point passes
    good = _g1_t(GP.G)
    assert g1.eq(good, g1.gen)
    ret, untouched = _raw_call(hip, pts[:7] + [good], 8, 1)
    assert ret == 0 and not untouched
    for n in (3, 6, 16384):
        assert _raw_call(hip, pts, n, 1) == (BADARGS, True), n
    for label in ("generic", "T11_0", "Q+T10177", "T3"):
        bad = _g1_t(GP.by_label(label).point)
        assert not GP.in_g1(GP.by_label(label).point)
        for pos in (0, 7, 15):
            p = list(pts)
            p[pos] = bad
            assert _raw_call(hip, p, 8, 2) == (BADARGS, True), (label, pos)
            assert _raw_call(hip, p, 16, 1, 1) == (BADARGS, True), (label, pos)
    off = _g1_t((1, 1))
    assert not GP.on_curve((1, 1))
    p = list(pts)
    p[9] = off
    assert _raw_call(hip, p, 16, 1) == (BADARGS, True)
    f = hip.lib.ckzg_hip_g1_fft
    f.restype = C.c_int
    assert f(None, b"".join(pts), C.c_uint64(16), C.c_uint64(1), C.c_int(0), hip.sp) == BADARGS
    assert f(C.create_string_buffer(16 * 144), None, C.c_uint64(16), C.c_uint64(1), C.c_int(0), hip.sp) == BADARGS
