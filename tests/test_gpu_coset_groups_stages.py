"""The four device stages of ckzg_hip_verify_coset_kzg_proof_batch_groups (csrc/coset_groups.hip) at every coset size
l = 2^e, read off the device whole -- data and a guard region on either side -- and compared exactly with Python integers
(tests/coset_groups_expect.py; libcoset_groups_shim.so: tests/native/coset_groups_shim.hip linked with the product's own
objects, so the kernels and the index maps are the product's):

  * k_coset_group_rlc_scalars + k_group_commit_weights: the powers buffer and the whole scalar buffer of the jobs, zeros
    on padding terms and on the terms another stage writes, with both paddings of the jobs;
  * k_coset_group_aggregate: the rows, at row counts on both sides of a workgroup of 256 slots and at the most parts;
  * k_coset_group_interp: the rows' coefficients with the coset factors taken out, in place;
  * k_coset_group_interp_sum: minus each group's sum onto its setup terms and nothing else, also split into parts.

Every stage gets the EXPECTED output of the stage before it as its input.  After any non-zero return of a shim call every
later test of the module fails at once without launching anything."""
import ctypes as C
import os
import random
import subprocess

import pytest

import coset_groups_expect as gx
import rlc_expect as rx
from conftest import ROOT

pytestmark = pytest.mark.gpu

R = gx.R
COSET_GROUPS_SHIM_SO = os.path.abspath(os.environ["CKZG_COSET_GROUPS_SHIM_SO"]) if os.environ.get("CKZG_COSET_GROUPS_SHIM_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "libcoset_groups_shim.so")
GUARD_VAL = int.from_bytes(bytes([0x5a]) * 32, "little")   # < r: survives the conversions of a Montgomery buffer
ES = list(range(7))
_broken = []


class CgsChunk(C.Structure):
    _fields_ = [("start", C.POINTER(C.c_uint64)), ("G", C.c_uint64), ("item_commit", C.POINTER(C.c_uint32)),
                ("num_commits", C.c_uint64), ("coset_indices", C.POINTER(C.c_uint64)), ("e", C.c_int32),
                ("quad_max_terms", C.c_uint64)]


class Shim:
    def __init__(self, lib):
        self.lib = lib
        self.guard = lib.cgs_guard()

    def call(self, fn, *args):
        if _broken:
            pytest.fail("an earlier shim call failed (%s): nothing more is launched" % _broken[0])
        rc = C.c_int(0)
        ret = getattr(self.lib, fn)(*args, C.byref(rc))
        if ret != 0 or rc.value != 0:
            _broken.append("%s -> %d, stage %d" % (fn, ret, rc.value))
            pytest.fail(_broken[0])


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(COSET_GROUPS_SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libcoset_groups_shim.so"])
    lib = C.CDLL(COSET_GROUPS_SHIM_SO)
    for fn in ("cgs_plan_info", "cgs_rlc_scalars", "cgs_aggregate", "cgs_interp", "cgs_interp_sum"):
        getattr(lib, fn).restype = C.c_int
    lib.cgs_guard.restype = C.c_size_t
    return Shim(lib)


@pytest.fixture(scope="module")
def roots():
    return rx.le32(gx.roots8193())


class Chunk:
    """a chunk as the shim takes it, with the values and challenges of its test"""

    def __init__(self, e, groups, seed, quad_max=8192):
        rnd = random.Random(seed)
        self.e, self.l = e, 1 << e
        self.sizes = [len(g) for g in groups]
        self.cols = [c for g in groups for c in g]
        n = self.n = len(self.cols)
        self.num_commits = min(3, n)
        self.item_commit = [i % self.num_commits if i < self.num_commits else rnd.randrange(self.num_commits) for i in range(n)]
        self.values = [[rnd.randrange(R) for _ in range(self.l)] for _ in range(n)]
        self.rs = [rnd.randrange(R) for _ in groups]
        G = len(groups)
        self._start = (C.c_uint64 * (G + 1))(*[sum(self.sizes[:g]) for g in range(G + 1)])
        self._commit = (C.c_uint32 * n)(*self.item_commit)
        self._cols = (C.c_uint64 * n)(*self.cols)
        self.c = CgsChunk(self._start, G, self._commit, self.num_commits, self._cols, e, quad_max)
        self.row_grp, self.row_col, self.item_row = gx.rows_of(self.sizes, self.cols)
        self.nrows = len(self.row_col)

    def info(self, shim):
        info = (C.c_uint32 * 6)()
        if _broken:
            pytest.fail("an earlier shim call failed (%s): nothing more is launched" % _broken[0])
        assert shim.lib.cgs_plan_info(info, C.byref(self.c)) == 0
        return list(info)


def _guarded(shim, vals):
    g = [GUARD_VAL] * shim.guard
    return C.create_string_buffer(rx.le32(g + list(vals) + g))


def _read(shim, buf, n):
    got = rx.from_le32(buf, n + 2 * shim.guard)
    g = [GUARD_VAL] * shim.guard
    assert got[:shim.guard] == g, "the guard in front of the data was written"
    assert got[shim.guard + n:] == g, "the guard behind the data was written"
    return got[shim.guard:shim.guard + n]


def _shape(e, nrows):
    """groups of coset indices with exactly nrows distinct (group, coset) rows: a coset twice in one group (one row of two
    items), an empty group between two others, the same coset in two groups (two rows), cosets 0, m - 1 and (from four
    rows on) 1, the rest spread over two more groups"""
    m = 8192 >> e
    assert 3 <= nrows <= m
    groups = [[0, m - 1, 0], [], [0] if nrows == 3 else [0, 1]]
    rest = [2 + i for i in range(nrows - 4)]
    if rest:
        groups += [rest[:len(rest) // 3], rest[len(rest) // 3:]]
    return [g for i, g in enumerate(groups) if g or i == 1]


def _stages(shim, roots, ch, what=("scalars", "aggregate", "interp", "sum")):
    e, l, n = ch.e, ch.l, ch.n
    info = ch.info(shim)
    per = 8 if info[1] else 32
    assert info[3] == ch.nrows
    if "scalars" in what or "sum" in what:
        want = gx.group_terms(ch.sizes, ch.item_commit, ch.num_commits, ch.cols, ch.values, ch.rs, e, per)
        total = len(want[0])
        assert info[0] == total
    first = gx.setup_terms(ch.sizes, ch.item_commit, e, per)
    setup = {t for f in first if f is not None for t in range(f, f + l)}
    rp = gx.powers(ch.sizes, ch.rs)
    rows_agg = gx.rows_aggregate(ch.sizes, ch.cols, ch.values, rp, e)
    rows_int = gx.rows_interp(rows_agg, ch.row_col, e)
    if "scalars" in what:
        rp_buf, sc_buf = _guarded(shim, [1] * n), _guarded(shim, [0] * total)
        shim.call("cgs_rlc_scalars", rp_buf, sc_buf, C.byref(ch.c), rx.le32(ch.rs), roots)
        assert _read(shim, rp_buf, n) == rp
        got = _read(shim, sc_buf, total)
        for t in range(total):
            assert got[t] == (0 if t in setup else want[1][t]), "term %d" % t
    if "aggregate" in what:
        rows_buf = _guarded(shim, [3] * (ch.nrows * l))
        shim.call("cgs_aggregate", rows_buf, rx.le32(v for it in ch.values for v in it), rx.le32(rp), C.byref(ch.c))
        assert _read(shim, rows_buf, ch.nrows * l) == rows_agg
    if "interp" in what:
        rows_buf = _guarded(shim, rows_agg)
        shim.call("cgs_interp", rows_buf, C.byref(ch.c), roots)
        assert _read(shim, rows_buf, ch.nrows * l) == rows_int
    if "sum" in what:
        sc_buf = _guarded(shim, [7] * total)
        shim.call("cgs_interp_sum", sc_buf, rx.le32(rows_int), C.byref(ch.c))
        got = _read(shim, sc_buf, total)
        for t in range(total):
            assert got[t] == (want[1][t] if t in setup else 7), "term %d" % t
    return info


@pytest.mark.parametrize("e,side", [(e, side) for e in ES for side in (-1, 0, 1)])
def test_stages_around_a_workgroup_of_256_slots(shim, roots, e, side):
    """R l = 256 - l, 256 and 256 + l"""
    ch = Chunk(e, _shape(e, (256 >> e) + side), 7000 + 10 * e + side)
    assert ch.nrows * ch.l == 256 + side * ch.l
    _stages(shim, roots, ch)


@pytest.mark.parametrize("e", ES)
def test_scalars_with_jobs_of_32_terms(shim, roots, e):
    """the other padding of the jobs: no four-lane ladders"""
    ch = Chunk(e, _shape(e, 5), 7100 + e, quad_max=0)
    assert ch.info(shim)[1] == 0
    _stages(shim, roots, ch, what=("scalars", "sum"))


@pytest.mark.parametrize("e", ES)
def test_aggregate_at_the_most_parts(shim, roots, e):
    """70 items on one coset and a group of one item: 16 parts by the rule of coset_verify_agg_parts over two rows, and
    lanes that take several items"""
    m = 8192 >> e
    ch = Chunk(e, [[m - 1] * 70, [1]], 7200 + e)
    info = _stages(shim, roots, ch, what=("aggregate",))
    assert info[3] == 2 and info[4] == 16


@pytest.mark.parametrize("e", ES)
def test_interp_sum_split_into_parts(shim, roots, e):
    """a group of 80 rows next to a group of one: two parts, and forty rows a lane -- more than one pass"""
    ch = Chunk(e, [list(range(80)), [0]], 7300 + e)
    info = _stages(shim, roots, ch, what=("interp", "sum"))
    assert info[3] == 81 and info[5] == 2
