"""The device stages of ckzg_hip_verify_coset_kzg_proof_batch read off the GPU and compared EXACTLY with Python integers
(tests/coset_verify_expect.py), at every coset size 2^e, through tests/native/coset_verify_shim.hip
(libcoset_verify_shim.so: the product's object files behind a C ABI): the scalars of the combination for a chosen r, the
aggregate, each column's coefficients and the sum over the columns.  Every buffer a stage writes goes up pre-filled with
a guard in front of the data and one behind it, and the whole of it is compared.  The inputs are the smallest at which
the lane mapping, the split of a long column, the fold and the bit reversal can go wrong: every column empty but one;
a column of 1, of 2 and of parts * k + 1 items; items on the columns 0 and m - 1; the values 0 and r - 1.  At e = 6, the
size verify_cell_kzg_proof_batch runs them at, also on the cases of the cell tests in tests/test_gpu_rlc_stages.py and
tests/test_gpu_poly_stages.py (which reach the same stages through the older entries of their shims, without guards in
front): every challenge of rlc_expect with member lists of 1 .. 107 cells, parts = 1 .. 16 on uniform and skewed columns,
128 columns of class vectors taken as values.

After any non-zero return of a shim call (a HIP error or the shim's 20 s deadline) every later test of the module
fails at once without launching anything."""
import ctypes as C
import os
import random
import subprocess

import pytest

import coset_verify_expect as V
import poly_expect as px
import rlc_expect as rx
from rlc_expect import R
from conftest import ROOT, SHIM_SO
from test_gpu_poly_stages import column_layouts, derangement
from test_gpu_rlc_stages import CHALLENGES, _member_lists

pytestmark = pytest.mark.gpu

CVS_SO = os.path.join(ROOT, "c-kzg-4844_amd", "libcoset_verify_shim.so")
FUNCTIONS = ["cvs_rlc_scalars", "cvs_aggregate", "cvs_interp"]
PAT = int.from_bytes(b"\xa5" * 32, "little") % R
SZ = C.c_size_t
ES = list(range(7))


class Shim:
    """libcoset_verify_shim.so; remembers the first failed call and refuses every later one"""

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
    if not os.path.exists(CVS_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libcoset_verify_shim.so"])
    lib = C.CDLL(CVS_SO)
    for fn in FUNCTIONS:
        getattr(lib, fn).restype = C.c_int
    lib.cvs_guard.restype = SZ
    return Shim(lib)


@pytest.fixture(scope="module")
def G(shim):
    return shim.lib.cvs_guard()


@pytest.fixture(scope="module")
def roots_raw():
    roots = rx.roots_of_unity()
    assert roots[:8192] == V.roots()
    return rx.le32(roots)


@pytest.fixture(scope="module")
def constants():
    what = (C.c_uint64 * 6)()
    C.CDLL(SHIM_SO).hs_coset_verify_constants(what)
    return dict(zip(("per_lane", "max_parts", "hash_on_pool_from", "min_shard", "agg_slots", "interp_threads"), what))


def guard(n, salt=0):
    """n canonical values no stage produces by accident"""
    return [(PAT + salt + i) % R for i in range(n)]


def fr_buf(vals):
    return C.create_string_buffer(rx.le32(vals), 32 * len(vals))


def u32(vals):
    return (C.c_uint32 * len(vals))(*vals)


def same(got, want, what):
    assert len(got) == len(want), what
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        pytest.fail("%s: element %d of %d is %x, expected %x" % (what, at, len(want), got[at], want[at]))


def csr(keys, nrows):
    """start [nrows + 1], order [n]: the indices of each row, ascending"""
    start = [0] * (nrows + 1)
    for k in keys:
        start[k + 1] += 1
    for t in range(nrows):
        start[t + 1] += start[t]
    fill, order = list(start[:nrows]), [0] * len(keys)
    for i, k in enumerate(keys):
        order[fill[k]] = i
        fill[k] += 1
    return start, order


def _values(rnd, l):
    ys = [rnd.randrange(R) for _ in range(l)]
    ys[rnd.randrange(l)] = rnd.choice((0, R - 1))
    return ys


def scenarios(e, constants):
    """name -> list of (commitment label, coset, values): the model's items without proofs"""
    rnd = random.Random(1000 + e)
    l, m = 1 << e, 8192 >> e
    mid = rnd.randrange(2, m - 2)
    out = {"one item, every other column empty": [(0, mid, _values(rnd, l))],
           "columns 0 and m - 1, a column of two": [(0, 0, _values(rnd, l)), (1, mid, _values(rnd, l)), (0, m - 1, [R - 1] * l),
                                                     (1, mid, _values(rnd, l)), (2, 1, [0] * l)]}
    # the first size at which a column is split over two lanes per slot: one column of 2 * 3 + 1 items, the others level
    n = m * constants["per_lane"] + 1
    cols = [mid] * 7 + [c % m for c in range(n - 7)]
    rnd.shuffle(cols)
    out["two parts, a column of 2 k + 1 items"] = [(i % 3, c, _values(rnd, l)) for i, c in enumerate(cols)]
    return out


def _items(sc):
    return [(cm, c, ys, None) for cm, c, ys in sc]


# ---- stage 2: the scalars ----

@pytest.mark.parametrize("e", ES)
def test_scalars(shim, G, roots_raw, e):
    rnd = random.Random(20 + e)
    m = 8192 >> e
    n = 131                                                     # three workgroups, the last one partly filled
    cosets = [0, m - 1, 1] + [rnd.randrange(m) for _ in range(n - 3)]
    commit = [0, 1, 0, 2] + [rnd.randrange(3) for _ in range(n - 4)]
    items = [(cm, c, [], None) for cm, c in zip(commit, cosets)]
    for r in (rnd.randrange(2, R), R - 1, 1, 0):
        want_rp, want_wrp, want_w = V.scalars(items, r, e)
        start, members = csr(commit, 3)
        rp, vrp, vwrp = (fr_buf(guard(n + 2 * G, s)) for s in (1, 2, 3))
        vw = fr_buf(guard(3 + 2 * G, 4))
        assert shim.call("cvs_rlc_scalars", rp, vrp, vwrp, vw, u32(cosets), u32(start), u32(members), fr_buf([r]), roots_raw,
                         SZ(n), SZ(3), e) == 0
        for buf, want, s, what in ((rp, want_rp, 1, "r^i"), (vrp, want_rp, 2, "r^i as scalars"), (vwrp, want_wrp, 3, "r^i x_c^l")):
            g = guard(n + 2 * G, s)
            same(rx.from_le32(buf, n + 2 * G), g[:G] + want + g[G + n:], what)
        g = guard(3 + 2 * G, 4)
        same(rx.from_le32(vw, 3 + 2 * G), g[:G] + want_w + g[G + 3:], "weights")


# ---- stages 3 to 5 ----

@pytest.mark.parametrize("e", ES)
def test_aggregate_coefficients_and_sum(shim, G, roots_raw, constants, e):
    l, m = 1 << e, 8192 >> e
    rnd = random.Random(40 + e)
    for name, sc in scenarios(e, constants).items():
        items, n = _items(sc), len(sc)
        r = rnd.randrange(2, R)
        rp = [pow(r, i, R) for i in range(n)]
        want_agg = V.aggregate(items, rp, e)
        start, order = csr([it[1] for it in items], m)
        # stage 3
        g = guard(8192 + 2 * G, 5)
        agg = fr_buf(g)
        flat = [y for it in items for y in it[2]]
        assert shim.call("cvs_aggregate", agg, fr_buf(flat), fr_buf(rp), u32(start), u32(order), SZ(n), e) == 0, name
        same(rx.from_le32(agg, 8192 + 2 * G), g[:G] + want_agg + g[G + 8192:], "aggregate: " + name)
        # stages 4 and 5 on what stage 3 left
        check_interp(shim, G, roots_raw, constants, agg, g, want_agg, e, name)


def check_interp(shim, G, roots_raw, constants, agg, g, want_agg, e, name):
    """cvs_interp on the buffer agg (the guard g around the aggregate want_agg): coefficients, partial rows and sum"""
    l = 1 << e
    per_block = constants["interp_threads"]
    nblocks = 8192 // per_block
    want_coeffs = V.columns_coeffs(want_agg, e)
    cols_per_block = per_block // l
    want_partial = [v for b in range(nblocks) for v in V.fold(want_coeffs, e, b * cols_per_block, (b + 1) * cols_per_block)]
    want_interp = V.interp_sum(want_agg, e)
    assert want_interp == [sum(want_partial[b * l + k] for b in range(nblocks)) % R for k in range(l)]
    gi, gp = guard(l + 2 * G, 6), guard(nblocks * l + 2 * G, 7)
    interp, partial = fr_buf(gi), fr_buf(gp)
    assert shim.call("cvs_interp", interp, partial, agg, roots_raw, e) == 0, name
    same(rx.from_le32(agg, 8192 + 2 * G), g[:G] + want_coeffs + g[G + 8192:], "coefficients: " + name)
    same(rx.from_le32(partial, nblocks * l + 2 * G), gp[:G] + want_partial + gp[G + nblocks * l:], "partial sums: " + name)
    same(rx.from_le32(interp, l + 2 * G), gi[:G] + want_interp + gi[G + l:], "sum over the columns: " + name)


@pytest.mark.parametrize("e", [3, 6])
def test_aggregate_at_the_most_parts(shim, G, constants, e):
    """every item on ONE column, enough of them for the widest split: 16 lanes per slot, each with several items (the
    number of items that takes grows with the number of columns: 262,152 values at e = 3, 262,208 at e = 6)"""
    l, m = 1 << e, 8192 >> e
    parts = constants["max_parts"]
    n = (parts // 2) * m * constants["per_lane"] + 1
    assert V.agg_parts(n, e, constants["per_lane"], parts) == parts and V.agg_parts(n - 1, e, constants["per_lane"], parts) == parts // 2
    rnd = random.Random(70 + e)
    c = m - 1
    base = [_values(rnd, l) for _ in range(5)]
    items = [(0, c, base[i % 5], None) for i in range(n)]
    r = rnd.randrange(2, R)
    rp = [pow(r, i, R) for i in range(n)]
    want = [0] * 8192
    for j in range(l):
        want[c * l + j] = sum(p * base[i % 5][j] for i, p in enumerate(rp)) % R
    start, order = csr([c] * n, m)
    g = guard(8192 + 2 * G, 8)
    agg = fr_buf(g)
    assert shim.call("cvs_aggregate", agg, fr_buf([y for it in items for y in it[2]]), fr_buf(rp), u32(start), u32(order), SZ(n), e) == 0
    same(rx.from_le32(agg, 8192 + 2 * G), g[:G] + want + g[G + 8192:], "aggregate")


# ---- the stages as verify_cell_kzg_proof_batch runs them: e = 6, 128 columns of 64 ----

CELL_E = 6


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_cell_rlc_scalars(shim, G, roots_raw, n):
    roots = rx.roots_of_unity()
    rnd = random.Random(7000 + n)
    cols = [(37 * i + 5) % 128 for i in range(n)]       # every one of the 128 columns at n = 300
    assert n < 300 or set(cols) == set(range(128))
    lists = _member_lists(rnd, n)
    assert n < 300 or [len(m) for m in lists] == [1, 63, 64, 65, 107]
    nc = len(lists)
    start = [0]
    for m in lists:
        start.append(start[-1] + len(m))
    members = [i for m in lists for i in m]
    assert sorted(members) == list(range(n))
    for r in CHALLENGES:
        rp, vrp, vwrp = (fr_buf(guard(n + 2 * G, s)) for s in (1, 2, 3))
        vw = fr_buf(guard(nc + 2 * G, 4))
        assert shim.call("cvs_rlc_scalars", rp, vrp, vwrp, vw, u32(cols), u32(start), u32(members), fr_buf([r]), roots_raw,
                         SZ(n), SZ(nc), CELL_E) == 0
        pw = [pow(r, i, R) for i in range(n)]
        for buf, want, s, what in ((rp, pw, 1, "d_rp"), (vrp, pw, 2, "vec_rp"),
                                   (vwrp, [pw[i] * roots[64 * rx.brev7(cols[i])] % R for i in range(n)], 3, "vec_wrp")):
            g = guard(n + 2 * G, s)
            same(rx.from_le32(buf, n + 2 * G), g[:G] + want + g[G + n:], "%s, r = %x" % (what, r))
        g = guard(nc + 2 * G, 4)
        same(rx.from_le32(vw, nc + 2 * G), g[:G] + [sum(pw[i] for i in m) % R for m in lists] + g[G + nc:],
             "commitment weights, r = %x" % r)


AGG_PARTS = {1: 1, 512: 1, 513: 2, 1025: 4, 2049: 8, 4097: 16}


@pytest.mark.parametrize("n", list(AGG_PARTS))
def test_cell_aggregate(shim, G, n):
    assert C.CDLL(SHIM_SO).hs_coset_verify_agg_parts(C.c_uint64(n), CELL_E) == AGG_PARTS[n]
    rnd = random.Random(7100 + n)
    cell_fr = [[rnd.getrandbits(254) for _ in range(64)] for _ in range(n)]
    if n > 1:
        cell_fr[1] = [0, 1, R - 1] + cell_fr[1][3:]
        cell_fr[n - 1] = [R - 1] * 64
    rp = px.values(rnd, n)
    order = derangement(rnd, n)
    flat, rp_buf = fr_buf([v for c in cell_fr for v in c]), fr_buf(rp)
    for name, col_start in column_layouts(n).items():
        assert col_start[128] == n and (name == "uniform" or n == 1 or col_start[78] - col_start[77] > n // 2)
        g = guard(8192 + 2 * G, 12)
        agg = fr_buf(g)
        assert shim.call("cvs_aggregate", agg, flat, rp_buf, u32(col_start), u32(order), SZ(n), CELL_E) == 0
        want = [v for row in px.cell_aggregate(cell_fr, rp, col_start, order) for v in row]
        same(rx.from_le32(agg, 8192 + 2 * G), g[:G] + want + g[G + 8192:], "n = %d, %s columns" % (n, name))


def test_interp_sum(shim, G, roots_raw, constants):
    rnd = random.Random(7200)
    cols = [px.class_vector(rnd, c, 64) for c in range(128)]
    values = [v for c in cols for v in c]
    g = guard(8192 + 2 * G, 13)
    agg = fr_buf(g[:G] + values + g[G + 8192:])
    check_interp(shim, G, roots_raw, constants, agg, g, values, CELL_E, "128 columns of class vectors")
