"""The device stages of ckzg_hip_recover_cosets_and_kzg_proofs_rows that depend on the coset size, read off the GPU and
compared EXACTLY with Python integers (tests/coset_recover_expect.py), through tests/native/coset_recover_shim.hip
(libcoset_recover_shim.so: the product's object files behind a C ABI): Z and 1 / Z of several sets in one launch at every
e and with every `parts` the picker can return (the shim passes it), the per-coset multiplication and the scatter.
Every buffer a stage writes goes up pre-filled with a guard in front of the data and one behind it, and the whole of it is
compared.  The sets: the two half sets with their closed forms, a set with no missing coset (both factors 1), counts
below `parts` and no multiple of it, and a random half.  At e <= 2 the random half is compared on a sample of cosets (its
full product is up to 67 M big-integer multiplications); every other set on all m.

After any non-zero return of a shim call (a HIP error or the shim's 20 s deadline) every later test of the module fails
at once without launching anything."""
import ctypes as C
import os
import random
import subprocess

import pytest

import coset_recover_expect as X
from coset_recover_expect import R
from conftest import ROOT, SHIM_SO

pytestmark = pytest.mark.gpu

CRS_SO = os.path.join(ROOT, "c-kzg-4844_amd", "libcoset_recover_shim.so")
PAT = int.from_bytes(b"\xa5" * 32, "little") % R
SZ = C.c_size_t
ES = list(range(7))


class Shim:
    """libcoset_recover_shim.so; remembers the first failed call and refuses every later one"""

    def __init__(self, lib):
        self.lib = lib
        self.dead = None

    def call(self, name, *args):
        if self.dead is not None:
            pytest.fail("an earlier shim call (%s) returned %d: nothing is launched any more" % self.dead)
        rc = C.c_int(-1)
        run = getattr(self.lib, name)(*args, C.byref(rc))
        if run != 0:
            self.dead = (name, run)
            pytest.fail("%s returned %d" % (name, run))
        return rc.value


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(CRS_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libcoset_recover_shim.so"])
    lib = C.CDLL(CRS_SO)
    for fn in ("crs_factors", "crs_mul_factor", "crs_scatter"):
        getattr(lib, fn).restype = C.c_int
    lib.crs_guard.restype = SZ
    return Shim(lib)


@pytest.fixture(scope="module")
def G(shim):
    return shim.lib.crs_guard()


@pytest.fixture(scope="module")
def roots_raw():
    return X.le32(X.roots())


def guard(n, salt=0):
    """n canonical values no stage produces by accident"""
    return [(PAT + salt + i) % R for i in range(n)]


def fr_buf(vals):
    return C.create_string_buffer(X.le32(vals), 32 * len(vals))


def fr_read(buf):
    raw = buf.raw
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def u32(vals):
    return (C.c_uint32 * max(len(vals), 1))(*vals)


def same(got, want, what):
    assert len(got) == len(want), what
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        pytest.fail("%s: element %d of %d is %x, expected %x" % (what, at, len(want), got[at], want[at]))


_EXPECT = {}


def factor_sets(e):
    """[(name, missing cosets, cosets compared, Z, 1 / Z)], made once per e"""
    if e in _EXPECT:
        return _EXPECT[e]
    m = 8192 >> e
    rnd = random.Random(300 + e)
    every = list(range(m))
    out = []
    for first in (True, False):
        missing = list(range(m // 2)) if first else list(range(m // 2, m))
        forms = [X.closed_form(first, c, e) for c in every]
        out.append(("first_half" if first else "second_half", missing, every, [d for d, _ in forms],
                    [pow(s, R - 2, R) for _, s in forms]))
    out.append(("none", [], every, [1] * m, [1] * m))
    for name, count in (("few", 37), ("three", 3)):
        missing = sorted(rnd.sample(range(m), count))
        out.append((name, missing, every) + X.factors(missing, every, e))
    missing = sorted(rnd.sample(range(m), m // 2))
    which = every if e >= 3 else sorted(set([0, m - 1, missing[0], missing[-1]] + rnd.sample(range(m), 64)))
    out.append(("random_half", missing, which) + X.factors(missing, which, e))
    _EXPECT[e] = out
    return out


def test_the_forced_parts_are_the_pickers():
    """every `parts` forced below is one the product's picker returns for some number of sets, and no other exists"""
    h = C.CDLL(SHIM_SO)
    h.hs_coset_recover_parts.restype = C.c_uint32
    for e in ES:
        got = {h.hs_coset_recover_parts(C.c_uint64(s), C.c_int(e)) for s in range(1, 1100)}
        assert sorted(got) == X.all_parts(e)


@pytest.mark.parametrize("e", ES)
def test_factors_of_several_sets_in_one_launch(shim, G, roots_raw, e):
    m = 8192 >> e
    sets = factor_sets(e)
    miss, start = [], [0]
    for _, missing, _, _, _ in sets:
        miss += [X.root_index(j, e) for j in missing]
        start.append(len(miss))
    n = len(sets) * m
    seven_l = C.create_string_buffer(X.le32([pow(7, 1 << e, R)]), 32)
    for parts in X.all_parts(e):
        pre_d, pre_i = guard(n + 2 * G, 1), guard(n + 2 * G, 7)
        zd, zi = fr_buf(pre_d), fr_buf(pre_i)
        rc = shim.call("crs_factors", zd, zi, u32(miss), u32(start), SZ(len(sets)), C.c_int(e), C.c_uint32(parts), roots_raw,
                       seven_l)
        assert rc == 0
        got_d, got_i = fr_read(zd), fr_read(zi)
        same(got_d[:G] + got_d[G + n:], pre_d[:G] + pre_d[G + n:], "guards of Z, parts %d" % parts)
        same(got_i[:G] + got_i[G + n:], pre_i[:G] + pre_i[G + n:], "guards of 1 / Z, parts %d" % parts)
        for s, (name, missing, which, want_d, want_i) in enumerate(sets):
            base = G + s * m
            same([got_d[base + c] for c in which], want_d, "Z of %s, parts %d" % (name, parts))
            same([got_i[base + c] for c in which], want_i, "1 / Z of %s, parts %d" % (name, parts))
            gone = set(missing)
            assert all((got_d[base + c] == 0) == (c in gone) for c in range(m)), name     # zero exactly on the missing cosets


def test_a_parts_the_stage_does_not_take(shim, G, roots_raw):
    n = 128
    zd, zi = fr_buf(guard(n + 2 * G)), fr_buf(guard(n + 2 * G))
    seven_l = C.create_string_buffer(X.le32([pow(7, 64, R)]), 32)
    for parts in (0, 3, 128):
        assert shim.call("crs_factors", zd, zi, u32([]), u32([0, 0]), SZ(1), C.c_int(6), C.c_uint32(parts), roots_raw, seven_l) != 0
    assert fr_read(zd) == guard(n + 2 * G)


@pytest.mark.parametrize("e", [0, 3, 6])
def test_multiplication_by_the_cosets_factor(shim, G, e):
    m, nrows, nsets = 8192 >> e, 3, 2
    rnd = random.Random(500 + e)
    row_set = [1, 0, 1]
    f = [rnd.randrange(R) for _ in range(nsets * m)]
    f[0], f[m - 1], f[m], f[2 * m - 1] = 0, R - 1, 1, 2
    a = [rnd.randrange(R) for _ in range(nrows * 8192)]
    pre = guard(G, 3) + a + guard(G, 4)
    buf = fr_buf(pre)
    assert shim.call("crs_mul_factor", buf, fr_buf(f), u32(row_set), SZ(nrows), SZ(nsets), C.c_int(e)) == 0
    want = pre[:G] + [a[g] * f[row_set[g >> 13] * m + ((g & 8191) >> e)] % R for g in range(len(a))] + pre[G + len(a):]
    same(fr_read(buf), want, "a *= f")


@pytest.mark.parametrize("e", [0, 3, 6])
def test_scatter_of_the_held_cosets(shim, G, e):
    m, nrows, item = 8192 >> e, 2, 32 << e
    rnd = random.Random(700 + e)
    dst = [0, nrows * m - 1, m - 1, m] + rnd.sample(range(1, nrows * m - 1), (nrows * m) // 3)
    dst = list(dict.fromkeys(dst))
    rnd.shuffle(dst)
    data = rnd.randbytes(len(dst) * item)
    pre = bytes([0x5a]) * (G * 32) + bytes(nrows * 8192 * 32) + bytes([0xc3]) * (G * 32)
    image = C.create_string_buffer(pre, len(pre))
    assert shim.call("crs_scatter", image, data, u32(dst), SZ(len(dst)), SZ(nrows), C.c_int(e)) == 0
    want = bytearray(pre)
    for i, d in enumerate(dst):
        want[G * 32 + d * item:G * 32 + (d + 1) * item] = data[i * item:(i + 1) * item]
    assert image.raw == bytes(want)
