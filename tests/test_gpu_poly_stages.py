"""The stages that move and combine vectors of Fr, read off the device and compared with integers.  Between the
arithmetic that tests/test_gpu_fields.py pins and the entry points that are compared with the oracle sits a layer
that end-to-end equality reaches only at the shapes and inputs the entry points happen to produce: six argument tuples
of the transform, a z nobody chooses (it is a hash), a divisor that is never zero, the `parts` a batch size happens to
select.  tests/native/poly_shim.hip (libpoly_shim.so: its entry file linked with the product's own object files, so the
kernels are the product's binary code) runs each stage on chosen inputs and returns its whole output buffer:

    fr_ntt_batch                                      k_ntt_tile<DIF / DIT>, k_ntt8192_outer<DIF / DIT>, inv_pow2
    bytes_to_fr_batch, fr_to_bytes_batch, zero_extend_batch
    eval_blob_bytes_batch_device                      the three launch forms of k_eval_tree
    eval_quotient_batch_device                        k_eval_barycentric<true>, k_quotient_in_domain
    fr_div_inplace_device, fr_mul_inplace_device      k_fr_div_inplace (zero divisors), k_fr_mul_inplace
    coset_recover_factors_enqueue, fr_mul_coset_factor_enqueue, scatter_cosets_rows_enqueue at cosets of 64; scatter_cells_device
    coset_aggregate_device, coset_group_aggregate_device at cosets of 64    parts = 1 .. 16
    coset_interp_device, coset_group_interp_device + coset_group_interp_sum_device at cosets of 64 (on the values of
    given coefficients)

Every comparison is exact and over the whole buffer, a guard region behind the data included: Python integers
(tests/poly_expect.py, each reference checked by a second route in tests/test_poly_expect_cpu.py) and bytes.

After any non-zero return of a shim call (a HIP error or the shim's 20 s deadline) every later test of the module
fails at once without launching anything."""
import ctypes as C
import itertools
import os
import random
import subprocess

import pytest

import poly_expect as px
import rlc_expect as rx
from rlc_expect import R
from conftest import ROOT

pytestmark = pytest.mark.gpu

# CKZG_POLY_SHIM_SO: another build of the shim (the way conftest.py takes CKZG_HIP_SO / CKZG_SHIM_SO)
POLY_SHIM_SO = os.path.abspath(os.environ["CKZG_POLY_SHIM_SO"]) if os.environ.get("CKZG_POLY_SHIM_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "libpoly_shim.so")
# every exported function this module binds (tests/test_poly_expect_cpu.py checks the library for them)
POLY_FUNCTIONS = ["ps_fr_ntt", "ps_bytes_to_fr", "ps_fr_to_bytes", "ps_zero_extend", "ps_eval_blob_bytes", "ps_eval_quotient",
                  "ps_fr_div_inplace", "ps_fr_mul_inplace", "ps_recover_set_factors", "ps_fr_mul_cell_factor", "ps_scatter_cells",
                  "ps_scatter_cells_rows", "ps_cell_aggregate", "ps_interp_sum", "ps_group_interp_sum"]
PAT = int.from_bytes(b"\xa5" * 32, "little") % R
SZ = C.c_size_t


class PolyShim:
    """libpoly_shim.so; remembers the first failed call and refuses every later one"""

    def __init__(self, lib):
        self.lib = lib
        self.dead = None

    def call(self, name, *args):
        """the stage's own return value (a refusal is a result); the call's return must be 0"""
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
    if not os.path.exists(POLY_SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libpoly_shim.so"])
    lib = C.CDLL(POLY_SHIM_SO)
    for fn in POLY_FUNCTIONS:
        getattr(lib, fn).restype = C.c_int
    return PolyShim(lib)


@pytest.fixture(scope="module")
def roots():
    return rx.roots_of_unity()


@pytest.fixture(scope="module")
def roots_raw(roots):
    return rx.le32(roots)


@pytest.fixture(scope="module")
def dom(roots):
    d = px.blob_domain(roots)
    return d, {w: i for i, w in enumerate(d)}


def guard(n, salt=0):
    """n canonical values no stage produces by accident"""
    return [(PAT + salt + i) % R for i in range(n)]


def fr_buf(vals):
    return C.create_string_buffer(rx.le32(vals), 32 * len(vals))


def u32(vals):
    return (C.c_uint32 * len(vals))(*vals)


def same(got, want, what):
    """whole-buffer equality with the first difference named"""
    assert len(got) == len(want), what
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        pytest.fail("%s: element %d of %d is %x, expected %x" % (what, at, len(want), got[at], want[at]))


# ---- 1. fr_ntt_batch ----

@pytest.mark.parametrize("logn", [1, 2, 6, 7, 11, 12, 13])
def test_fr_ntt_batch(shim, roots, roots_raw, logn):
    """two tiles' worth of transforms (three of 8192), each sub-vector of another value class, every (dif, inverse)
    pair with and without 1 / n; a guard tile behind the data comes back as sent"""
    n = 1 << logn
    count = 3 if logn == 13 else 2 * 4096 // n
    rnd = random.Random(1300 + logn)
    tile = guard(4096, logn)
    for p, (dif, inverse) in enumerate(itertools.product((1, 0), (0, 1))):
        vecs = [px.class_vector(rnd, p * count + v, n) for v in range(count)]
        plain = [px.ntt(v, roots, logn, dif, inverse, False) for v in vecs]
        for scale in (0, 1):
            buf = fr_buf([x for v in vecs for x in v] + tile)
            rc = shim.call("ps_fr_ntt", buf, SZ(count * n + 4096), roots_raw, SZ(count), logn, dif, inverse, scale)
            assert rc == 0
            want = [x for o in plain for x in (px.times_inv_n(o, logn) if scale else o)] + tile
            same(rx.from_le32(buf, count * n + 4096), want, "logn %d dif %d inverse %d scale %d" % (logn, dif, inverse, scale))


@pytest.mark.parametrize("count,logn,want_rc", [(3, 6, 2), (1, 14, 2), (0, 7, 0)])
def test_fr_ntt_batch_refusals(shim, roots_raw, count, logn, want_rc):
    """a batch that is no whole number of tiles and a size past 8192 are refused, an empty batch is nothing to do: the
    buffer comes back unchanged in each case"""
    n_elems = (count << logn) + 4096
    sent = guard(n_elems, 77)
    for dif, inverse, scale in ((1, 0, 0), (0, 1, 1)):
        buf = fr_buf(sent)
        rc = shim.call("ps_fr_ntt", buf, SZ(n_elems), roots_raw, SZ(count), logn, dif, inverse, scale)
        assert rc == want_rc
        same(rx.from_le32(buf, n_elems), sent, "count %d logn %d" % (count, logn))


# ---- 2. the byte conversions ----

NOT_CANONICAL = [R, R + 1, (1 << 256) - 1, R + (1 << 232)]


@pytest.mark.parametrize("epu", [1, 64, 4096])
def test_bytes_to_fr_batch(shim, epu):
    """a ragged last workgroup; values >= r at the first and last element of a unit and of the whole input, R - 1 next
    to each: the output is 0 exactly there, the flags are exact word for word, and a null d_bad changes nothing"""
    total = 4096 + 64 + 37
    rnd = random.Random(2100 + epu)
    vals = px.values(rnd, total)
    planted = sorted({0, epu - 1, epu % total, 4095, 4096, (total // epu) * epu % total, total - 1})
    for t, pos in enumerate(planted):
        for nb in (pos - 1, pos + 1):
            if 0 <= nb < total and nb not in planted:
                vals[nb] = R - 1
        vals[pos] = NOT_CANONICAL[t % 4]
    assert {vals[p] for p in planted} == set(NOT_CANONICAL)
    raw = b"".join(v.to_bytes(32, "big") for v in vals)
    n_bad = total + 8   # (at least elems_per_unit words: a flag at any index below that stays inside the buffer)
    want_out = [v if v < R else 0 for v in vals] + guard(256)
    want_bad = [0] * n_bad
    for pos in planted:
        want_bad[pos // epu] = 1
    outs = []
    for with_bad in (1, 0):
        out = fr_buf([PAT] * total + guard(256))
        bad = u32([0] * n_bad)
        rc = shim.call("ps_bytes_to_fr", out, SZ(total + 256), bad, SZ(n_bad), raw, SZ(total), C.c_uint32(epu), with_bad)
        assert rc == 0
        same(rx.from_le32(out, total + 256), want_out, "out, elems_per_unit %d, d_bad %s" % (epu, "given" if with_bad else "null"))
        same(list(bad), want_bad if with_bad else [0] * n_bad, "bad, elems_per_unit %d" % epu)
        outs.append(out.raw)
    assert outs[0] == outs[1]


def test_fr_to_bytes_batch(shim):
    total = 293
    vals = px.values(random.Random(2200), total)
    out = C.create_string_buffer(b"\xa5" * (32 * (total + 256)), 32 * (total + 256))
    rc = shim.call("ps_fr_to_bytes", out, SZ(32 * (total + 256)), rx.le32(vals), SZ(total))
    assert rc == 0
    assert out.raw == b"".join(v.to_bytes(32, "big") for v in vals) + b"\xa5" * (32 * 256)


@pytest.mark.parametrize("count,n_src,n_dst", [(3, 4096, 8192), (5, 64, 128)])
def test_zero_extend_batch(shim, count, n_src, n_dst):
    rnd = random.Random(2300 + count)
    src = px.values(rnd, count * n_src)
    sent = guard(count * n_dst + 256, 5)
    dst = fr_buf(sent)
    rc = shim.call("ps_zero_extend", dst, SZ(len(sent)), rx.le32(src), SZ(count), C.c_uint32(n_src), C.c_uint32(n_dst))
    assert rc == 0
    want = [x for v in range(count) for x in src[v * n_src:(v + 1) * n_src] + [0] * (n_dst - n_src)] + sent[count * n_dst:]
    same(rx.from_le32(dst, len(sent)), want, "count %d" % count)


# ---- 3. eval_blob_bytes_batch_device ----

LEAVES = [0, 3, 4, 63, 64, 2049, 4095]
DOMAIN_M = [0, 1, 2, 2047, 2048, 4095]


def special_zs(dom):
    """0, 1, R - 1, w_m and w_m + 1 for the m of DOMAIN_M, without repeats (w_0 = 1, w_1 = R - 1, w_1 + 1 = 0)"""
    out = []
    for z in [0, 1, R - 1] + [dom[m] for m in DOMAIN_M] + [(dom[m] + 1) % R for m in DOMAIN_M]:
        if z not in out:
            out.append(z)
    return out


# the leaves of each launch: all seven positions over the four launches, and in every launch leaves that sit in another
# lane, another wave (n = 7: sixteen leaves per thread) and the last thread, so that every level of the fold carries one
LAUNCH_LEAVES = {7: [3, 64, 2049, 4095], 257: [0, 63, 2049, 4095], 1031: [4, 64, 2049, 4095], 2049: [0, 63, 2049, 4095]}
# A polynomial of degree <= 7 is its own remainder at every node from the third level up: both children of such a node
# agree and the node's twiddle drops out.  The levels above are carried by the single leaves and by this polynomial,
# whose expected value is as cheap: a few terms up to the full degree.
SPARSE_EXPONENTS = [0, 1, 64, 2047, 2048, 4095]


def eval_items(n, dom, index):
    """the eight blobs of the launch of n items (lists of integers), each item's blob, its z and its expected y"""
    rnd = random.Random(3100 + n)
    pa = px.values(rnd, 8)
    sparse = [(rnd.randrange(1, R), e) for e in SPARSE_EXPONENTS]
    blobs = [[px.horner(pa, w) for w in dom], [px.sparse_eval(sparse, w) for w in dom], [0] * 4096, [R - 1] * 4096]
    kinds = [lambda z: px.horner(pa, z), lambda z: px.sparse_eval(sparse, z), lambda z: 0, lambda z: R - 1]
    assert sorted({p for v in LAUNCH_LEAVES.values() for p in v}) == LEAVES
    for t, pos in enumerate(LAUNCH_LEAVES[n]):
        leaf = [0] * 4096
        leaf[pos] = R - 1 if t == 0 else rnd.randrange(1, R)
        blobs.append(leaf)
        kinds.append(None)
    K = len(blobs)
    # n = 7 leaves the all-zero blob out: the seven items are both polynomials, the constant R - 1 and all four leaves
    item_blob = [0, 1, 3, 4, 5, 6, 7] if n == 7 else [(5 * i + i // K) % K for i in range(n)]
    sp = special_zs(dom)
    zs = []
    while len(zs) < n:
        z = rnd.randrange(R)
        if z not in sp and z not in index:
            zs.append(z)
    if n == 7:
        at = {i: sp[(2 * i) % (len(sp) - 1)] for i in range(7)}
    else:
        # the last items hold a special z: at n = 2049 these are 2048 (alone in the second turn, seven waves idle) and
        # 2047 (the last of the first turn)
        tail = [n - 1, n - 2, n - 3]
        at = {i: sp[i] for i in range(len(sp) - 3)}
        at.update({i: z for i, z in zip(tail, sp[-3:])})
    assert len(at) == min(n, len(sp))
    for i, z in at.items():
        zs[i] = z
    assert len(set(zs)) == n
    want = [kinds[b](z) if kinds[b] is not None else px.eval_form(blobs[b], z, dom, index) for b, z in zip(item_blob, zs)]
    return blobs, item_blob, zs, want


def blob_bytes(blob):
    return b"".join(v.to_bytes(32, "big") for v in blob)


@pytest.mark.parametrize("n", [7, 257, 1031, 2049])
def test_eval_blob_bytes(shim, roots_raw, dom, n):
    """four waves per polynomial (n < 256), one wave each with four per workgroup (n <= 1024), eight per workgroup and,
    at 2049 = 256 * 8 + 1, a second turn of workgroup 0 with one polynomial; z = 0, 1, -1, inside the domain, next to
    it and random; a polynomial of degree 7, one of a few terms up to degree 4095, the constants 0 and R - 1 and blobs
    with one non-zero leaf"""
    blobs, item_blob, zs, want = eval_items(n, *dom)
    y = fr_buf(guard(n + 8, 3))
    bad = u32([0] * (n + 8))
    rc = shim.call("ps_eval_blob_bytes", y, bad, SZ(n + 8), b"".join(blob_bytes(b) for b in blobs), SZ(len(blobs)), u32(item_blob),
                   rx.le32(zs), SZ(n), roots_raw)
    assert rc == 0
    same(rx.from_le32(y, n + 8), want + guard(n + 8, 3)[n:], "y, n = %d" % n)
    assert list(bad) == [0] * (n + 8)


def test_eval_blob_bytes_flags_exactly_the_items_with_an_element_out_of_range(shim, roots_raw, dom):
    blobs, _, zs, _ = eval_items(7, *dom)
    spoilt0, spoilt6 = list(blobs[0]), list(blobs[1])
    spoilt0[1234] = R
    spoilt6[4095] = (1 << 256) - 1
    use = [spoilt0] + blobs[3:8] + [spoilt6]
    item_blob = list(range(7))
    y = fr_buf(guard(7 + 8, 4))
    bad = u32([0] * (7 + 8))
    rc = shim.call("ps_eval_blob_bytes", y, bad, SZ(7 + 8), b"".join(blob_bytes(b) for b in use), SZ(7), u32(item_blob), rx.le32(zs),
                   SZ(7), roots_raw)
    assert rc == 0
    assert list(bad) == [1, 0, 0, 0, 0, 0, 1] + [0] * 8
    got = rx.from_le32(y, 15)
    assert got[1:6] == [px.eval_form(use[i], zs[i], *dom) for i in range(1, 6)]
    assert got[7:] == guard(15, 4)[7:]


# ---- 4. eval_quotient_batch_device ----

def quotient_items(dom):
    """13 (polynomial, z) pairs: z = 0, w_m at both parities and both ends, next to the domain, random; polynomials
    random, all R - 1, all 0, constant (q = 0), and random with p_i = y at two positions off m"""
    rnd = random.Random(4100)
    rand_poly = lambda: [rnd.randrange(R) for _ in range(4096)]
    zs = [0] + [dom[m] for m in (0, 1, 2, 511, 512, 4094, 4095)] + [(dom[3] + 1) % R] + [rnd.randrange(R) for _ in range(3)] + \
        [(dom[2048] + 1) % R]
    const = rnd.randrange(1, R)
    polys = [rand_poly(), rand_poly(), [R - 1] * 4096, rand_poly(), [0] * 4096, [const] * 4096, rand_poly(), rand_poly(),
             rand_poly(), [R - 1] * 4096, [const] * 4096, rand_poly(), [0] * 4096]
    for item, m, (a, b) in ((3, 2, (3, 4095)), (6, 4094, (0, 4093)), (7, 4095, (4094, 17))):
        assert zs[item] == dom[m]
        polys[item][a] = polys[item][b] = polys[item][m]
    return polys, zs


def test_eval_quotient_hits_and_misses_in_one_launch(shim, roots_raw, dom):
    d, index = dom
    polys, zs = quotient_items(d)
    n = len(zs)
    assert n == 13
    want = [px.quotient(p, z, d, index) for p, z in zip(polys, zs)]
    assert [w[1] for w in want] == [-1, 0, 1, 2, 511, 512, 4094, 4095, -1, -1, -1, -1, -1]
    y = fr_buf(guard(n + 1, 6))
    q_sent = b"\xa5" * (32 * 4096 * (n + 1))
    q = C.create_string_buffer(q_sent, len(q_sent))
    hit = (C.c_int32 * (n + 1))(*([0x5a5a5a5a] * (n + 1)))
    rc = shim.call("ps_eval_quotient", y, q, hit, rx.le32([v for p in polys for v in p]), rx.le32(zs), SZ(n), roots_raw)
    assert rc == 0
    assert list(hit) == [w[1] for w in want] + [0x5a5a5a5a]
    same(rx.from_le32(y, n + 1), [w[0] for w in want] + guard(n + 1, 6)[n:], "y")
    raw = q.raw
    for i in range(n):
        same(rx.from_le32(raw[32 * 4096 * i:32 * 4096 * (i + 1)], 4096), want[i][2], "q of item %d (hit %d)" % (i, want[i][1]))
    assert raw[32 * 4096 * n:] == q_sent[32 * 4096 * n:]


# ---- 5. in-place quotients and products ----

@pytest.mark.parametrize("n", [1, 15, 16, 17, 1029])
def test_fr_div_inplace(shim, n):
    """a / b, and 0 where b = 0 (blst's inverse of zero) with the rest of the run unharmed: a zero divisor at the first,
    a middle and the last place of a run, two adjacent ones, a run of nothing else, a partial last run"""
    rnd = random.Random(5100 + n)
    n_elems = (n + 15) // 16 * 16 + 16
    a = px.values(rnd, n) + guard(n_elems - n, 8)
    b = [rnd.randrange(1, R) for _ in range(n_elems)]
    zeros = {0, 16 + 7, 32 + 15, 52, 53, n - 1} | set(range(64, 80)) | ({7} if n == 15 else set())
    zeros = {i for i in zeros if i < n and n > 1}
    for i in zeros:
        b[i] = 0
    b[n_elems - 3] = 0   # (in the guard)
    if n > 1:
        b[1], a[1] = R - 1, R - 1
    buf = fr_buf(a)
    rc = shim.call("ps_fr_div_inplace", buf, rx.le32(b), SZ(n_elems), SZ(n))
    assert rc == 0
    want = [a[i] * pow(b[i], -1, R) % R if b[i] else 0 for i in range(n)] + a[n:]
    same(rx.from_le32(buf, n_elems), want, "n = %d" % n)


@pytest.mark.parametrize("n,period", [(8192 + 37, 64), (300, 300)])
def test_fr_mul_inplace(shim, n, period):
    rnd = random.Random(5200 + n)
    a = px.values(rnd, n) + guard(256, 9)
    b = px.values(rnd, period)
    buf = fr_buf(a)
    rc = shim.call("ps_fr_mul_inplace", buf, SZ(n + 256), rx.le32(b), SZ(n), SZ(period))
    assert rc == 0
    same(rx.from_le32(buf, n + 256), [a[i] * b[i % period] % R for i in range(n)] + a[n:], "n = %d" % n)


# ---- 6. recovery factors and scatters ----

def recover_sets():
    rnd = random.Random(6100)
    every = set(range(128))
    return [every, every - {0}, every - {127}, set(range(1, 128, 2)), set(range(64, 128)), every - set(rnd.sample(range(128), 40))]


def test_recover_set_factors(shim, roots, roots_raw):
    sets = recover_sets()
    assert [128 - len(s) for s in sets] == [0, 1, 1, 64, 64, 40]
    ns = len(sets)
    sent = guard((ns + 1) * 128, 10)
    zd, zi = fr_buf(sent), fr_buf(sent)
    rc = shim.call("ps_recover_set_factors", zd, zi, u32([w for s in sets for w in px.mask_words(s)]), SZ(ns), roots_raw)
    assert rc == 0
    want = [px.set_factors(s, roots) for s in sets]
    for s, (d, _) in zip(sets, want):
        assert [c for c in range(128) if d[c] == 0] == sorted(set(range(128)) - s)
    same(rx.from_le32(zd, len(sent)), [v for w in want for v in w[0]] + sent[ns * 128:], "z_domain")
    same(rx.from_le32(zi, len(sent)), [v for w in want for v in w[1]] + sent[ns * 128:], "z_coset_inv")


def test_fr_mul_cell_factor(shim):
    rnd = random.Random(6200)
    row_set = [2, 0, 2]
    f = px.values(rnd, 3 * 128)
    a = px.values(rnd, 3 * 8192) + guard(8192, 11)
    buf = fr_buf(a)
    rc = shim.call("ps_fr_mul_cell_factor", buf, rx.le32(f), SZ(3), u32(row_set), SZ(3))
    assert rc == 0
    want = [a[g] * f[row_set[g // 8192] * 128 + (g % 8192) // 64] % R for g in range(3 * 8192)] + a[3 * 8192:]
    same(rx.from_le32(buf, 4 * 8192), want, "rows")


def test_scatter_cells(shim):
    rnd = random.Random(6300)
    rows, nc = 3, 64
    idx = rnd.sample(range(128), nc)
    assert idx != sorted(idx)
    cells = rnd.randbytes(rows * nc * 2048)
    sent = b"\xa5" * ((rows + 1) * 128 * 2048)
    image = C.create_string_buffer(sent, len(sent))
    rc = shim.call("ps_scatter_cells", image, cells, u32(idx), C.c_uint32(nc), SZ(rows))
    assert rc == 0
    want = bytearray(sent)
    for b in range(rows):
        for j in range(nc):
            at = (b * 128 + idx[j]) * 2048
            want[at:at + 2048] = cells[(b * nc + j) * 2048:(b * nc + j + 1) * 2048]
    assert image.raw == bytes(want)


def test_scatter_cells_rows(shim):
    rnd = random.Random(6400)
    rows, nc = 3, 70
    dst = rnd.sample(range(rows * 128), nc)
    cells = rnd.randbytes(nc * 2048)
    size = (rows + 1) * 128 * 2048
    image = C.create_string_buffer(size)   # zero-filled, as the caller of the stage leaves it
    rc = shim.call("ps_scatter_cells_rows", image, SZ(rows), cells, u32(dst), SZ(nc))
    assert rc == 0
    want = bytearray(size)
    for i, d in enumerate(dst):
        want[d * 2048:(d + 1) * 2048] = cells[i * 2048:(i + 1) * 2048]
    assert image.raw == bytes(want)


# ---- 7. aggregation and interpolation ----

def derangement(rnd, n):
    """a permutation with order[t] != t (n > 1)"""
    order = list(range(n))
    while n > 1 and any(order[t] == t for t in range(n)):
        rnd.shuffle(order)
    return order


def column_layouts(n):
    """col_start[129] of the uniform layout and of the skewed one: columns 3 .. 9 and 100 .. 119 empty, column 77 with
    more than half of the cells"""
    uniform = [c * n // 128 for c in range(129)]
    big = n // 2 + 1
    open_cols = [c for c in range(128) if c != 77 and not 3 <= c <= 9 and not 100 <= c <= 119]
    sizes = [0] * 128
    sizes[77] = big
    for t in range(n - big):
        sizes[open_cols[(7 * t) % len(open_cols)]] += 1
    skewed = [sum(sizes[:c]) for c in range(129)]
    return {"uniform": uniform, "skewed": skewed}


def run_cell_aggregate(shim, cell_fr, rp, row_start, order, grouped):
    n, nrows = len(rp), len(row_start) - 1
    sent = guard((nrows + 1) * 64, 12)
    out = fr_buf(sent)
    rc = shim.call("ps_cell_aggregate", out, rx.le32([v for c in cell_fr for v in c]), rx.le32(rp), u32(row_start), u32(order), SZ(n),
                   SZ(nrows), grouped)
    assert rc == 0
    want = [v for row in px.cell_aggregate(cell_fr, rp, row_start, order) for v in row] + sent[nrows * 64:]
    return rx.from_le32(out, len(sent)), want


@pytest.mark.parametrize("n", [1, 512, 513, 1025, 2049, 4097])   # parts = 1, 1, 2, 4, 8, 16
def test_cell_aggregate(shim, n):
    rnd = random.Random(7100 + n)
    cell_fr = [[rnd.getrandbits(254) for _ in range(64)] for _ in range(n)]
    if n > 1:
        cell_fr[1] = [0, 1, R - 1] + cell_fr[1][3:]
        cell_fr[n - 1] = [R - 1] * 64
    rp = px.values(rnd, n)
    order = derangement(rnd, n)
    for name, col_start in column_layouts(n).items():
        assert col_start[128] == n and (name == "uniform" or n == 1 or col_start[78] - col_start[77] > n // 2)
        got, want = run_cell_aggregate(shim, cell_fr, rp, col_start, order, 0)
        same(got, want, "n = %d, %s columns" % (n, name))


def test_interp_sum(shim, roots, roots_raw):
    rnd = random.Random(7200)
    cols = [px.class_vector(rnd, c, 64) for c in range(128)]
    sent = guard(128, 13)
    out = fr_buf(sent)
    rc = shim.call("ps_interp_sum", out, rx.le32([v for c in cols for v in c]), roots_raw)
    assert rc == 0
    same(rx.from_le32(out, 128), px.interp_sum(cols, list(range(128)), roots) + sent[64:], "interp")


GROUP_ROWS = [0, 1, 5, 130]


def test_group_cell_aggregate(shim):
    """k_coset_group_aggregate at cosets of 64 over (group, column) rows: 136 rows of 0 .. 9 cells, parts = 2"""
    rnd = random.Random(7300)
    nrows = sum(GROUP_ROWS)
    sizes = [(7 * t + 3) % 10 for t in range(nrows)]
    n = sum(sizes)
    assert 0 in sizes and nrows * 4 < n <= 2 * nrows * 4
    row_start = [sum(sizes[:t]) for t in range(nrows + 1)]
    cell_fr = [px.values(rnd, 64) for _ in range(n)]
    rp = px.values(rnd, n)
    got, want = run_cell_aggregate(shim, cell_fr, rp, row_start, derangement(rnd, n), 1)
    same(got, want, "rows")


def test_group_interp_sum(shim, roots, roots_raw):
    """the index arrays by hand, to the layout coset_groups.hip documents: gd = start [G + 1] | first term of A_g [G] | distinct
    commitments of g [G] | first term of B_g [G]; A_g = commitments | proofs | 64 setup points.  The 64 setup terms of
    each non-empty group become -interp_g[k]; nothing else of sc changes, and the empty group writes nothing"""
    rnd = random.Random(7400)
    G = len(GROUP_ROWS)
    nrows = sum(GROUP_ROWS)
    grp_rows = [sum(GROUP_ROWS[:g]) for g in range(G + 1)]
    cells = [0, 3, 17, 600]          # cells per group: the empty group has none
    commits = [0, 2, 1, 5]           # distinct commitments per group
    start = [sum(cells[:g]) for g in range(G + 1)]
    pad8 = lambda v: (v + 7) // 8 * 8
    first_a, first_b, at = [], [], 0
    for g in range(G):
        first_a.append(at)
        at += pad8(commits[g] + cells[g] + 64) if cells[g] else 0
        first_b.append(at)
        at += pad8(cells[g])
    total = (at + 63) // 64 * 64 + 64   # (one more block of 64 terms: the guard)
    gd = start + first_a + commits + first_b
    assert len(gd) == 4 * G + 1
    row_col = [(37 * t + 11) % 128 for t in range(nrows)]
    rows = [px.class_vector(rnd, t, 64) for t in range(nrows)]
    sent = [rnd.getrandbits(256) for _ in range(total)]
    sc = fr_buf(sent)
    rc = shim.call("ps_group_interp_sum", sc, SZ(total), rx.le32([v for r in rows for v in r]), SZ(nrows), u32(grp_rows), u32(row_col),
                   u32(gd), SZ(G), roots_raw)
    assert rc == 0
    want = list(sent)
    for g in range(G):
        if not cells[g]:
            continue
        a, b = grp_rows[g], grp_rows[g + 1]
        interp = px.interp_sum(rows[a:b], row_col[a:b], roots)
        t0 = first_a[g] + commits[g] + cells[g]
        want[t0:t0 + 64] = [-v % R for v in interp]
    assert sum(1 for s, w in zip(sent, want) if s != w) == 3 * 64
    same(rx.from_le32(sc, total), want, "sc")
