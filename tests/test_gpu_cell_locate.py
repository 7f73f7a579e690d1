"""ckzg_hip_verify_cell_kzg_proof_batch_locate: one verify_cell_kzg_proof_batch verdict per cell, at the cost of one batch
check when every cell verifies.  Expected values come from the consensus-spec vectors, from the CPU oracle's
verify_cell_kzg_proof_batch on an item alone (once per distinct item), or from the existing
ckzg_hip_verify_cell_kzg_proof_batch_groups with groups of one -- never from the call under test.  The cells, proofs and
commitments of the built batches are the oracle's, of 8 blobs, as in test_gpu_cell_groups.py."""
import ctypes as C
import random
import re
import os

import pytest

import cell_locate_items as CL
import g1_points as GP
from kzg_ctypes import HIP_SO, Kzg
from test_gpu_cell_groups import _blob

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ckzg_hip_verify_cell_kzg_proof_batch_locate"
BADARGS = CL.BADARGS


def _chunk_cells():
    src = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    return int(re.search(r"#define CKZG_HIP_CELL_LOCATE_CHUNK_CELLS (\d+)", src).group(1))


@pytest.fixture(scope="module")
def material(oracle):
    """commitments, cells and proofs of 8 random blobs from the CPU oracle"""
    blobs = [_blob(83, i) for i in range(8)]
    cm = [oracle.blob_to_kzg_commitment(b) for b in blobs]
    cp = [oracle.compute_cells_and_kzg_proofs(b) for b in blobs]
    return cm, [c for c, _ in cp], [p for _, p in cp]


def _item(material, b, c):
    cm, cells, proofs = material
    return (cm[b], c, cells[b][c], proofs[b][c])


def _good(material, n):
    """n good items: blob i mod 8, column 7 i + 3 mod 128 (distinct (blob, column) pairs up to 128 items)"""
    return [_item(material, i % 8, (7 * i + 3) % 128) for i in range(n)]


def _run(api, items):
    return api.verify_cell_kzg_proof_batch_locate(*[[t[k] for t in items] for k in range(4)])


def _raw(api, items, with_status=True, with_stats=True, with_ok=True):
    n = len(items)
    f = getattr(api.lib, NAME)
    f.restype = C.c_int
    ok = (C.c_bool * max(n, 1))(*([True] * max(n, 1)))
    st = (C.c_uint8 * max(n, 1))(*([7] * max(n, 1)))
    stats = (C.c_uint64 * 3)(9, 9, 9)
    j = lambda k: b"".join(t[k] for t in items)
    ret = f(ok if with_ok else None, st if with_status else None, stats if with_stats else None, j(0),
            (C.c_uint64 * max(n, 1))(*[t[1] for t in items]), j(2), j(3), C.c_uint64(n), api.sp)
    return ret, [bool(v) for v in ok[:n]], [int(v) for v in st[:n]], [int(v) for v in stats]


def _groups_of_one(hip, items):
    """the existing road to a verdict per cell: (ok, status) per item"""
    ok, st = hip.verify_cell_kzg_proof_batch_groups([[[t[0]], [t[1]], [t[2]], [t[3]]] for t in items])
    return list(zip(ok, st))


def _expected(hip, oracle, items):
    if len(items) <= 65:
        return [CL.verdict(oracle, t) for t in items]
    return _groups_of_one(hip, items)


def _check(got, want, what=None):
    ok, st, stats = got
    assert len(ok) == len(want) and len(st) == len(want)
    for i, w in enumerate(want):
        assert (ok[i], st[i]) == w, (what, i, ok[i], st[i], w)
    n, f = len(want), want.count((False, 0))
    if all(w[1] for w in want):
        assert stats[0] == 0, (what, stats)
    elif f == 0:
        assert stats[0] == stats[2], (what, stats)   # one check per chunk
    else:
        assert 1 <= stats[0] <= stats[2] + 2 * f * CL.ceil_log2(n), (what, stats)
    return stats


# ---- the consensus vectors ----

def test_all_well_formed_spec_vectors_in_one_call(hip, oracle):
    items = CL.spec_items()
    assert len(items) == 925
    # a vector that verifies is made of items that verify; the items of the others are asked of the oracle one by one
    want = [(True, 0) if t[4] is True else CL.verdict(oracle, t) for t in items]
    assert set(want) == {(True, 0), (False, 0), (False, BADARGS)}
    ret, ok, st, stats = _raw(hip, items)
    assert ret == BADARGS
    stats = _check((ok, st, stats), want, "spec")
    assert stats[1] == 0 and stats[2] == 1
    # ... and in the opposite order
    _check(_run(hip, items[::-1]), want[::-1], "spec reversed")


# ---- built batches ----

def _defects(material, n):
    """(what, items): the good batch of n with defects of each kind"""
    cm, cells, proofs = material
    good = _good(material, n)
    p = n // 2
    c, x, k, q = good[p]
    b = p % 8
    out = [("good", good)]

    def one(what, item, at=p):
        items = list(good)
        items[at] = item
        out.append((what, items))

    one("bit flipped", (c, x, CL.flip_low_bit(k, 17), q))
    one("bit flipped in the last element", (c, x, CL.flip_low_bit(k, 63), q))
    one("proof of another cell", (c, x, k, proofs[b][(x + 1) % 128]))
    one("commitment of another blob", (cm[(b + 1) % 8], x, k, q))
    one("right cell under the wrong index", (c, (x + 1) % 128, k, q))
    if n >= 2:
        items = list(good)
        for at in (p - 1, p):   # (p = ceil(n / 2) for odd n - 1: around the middle)
            t = items[at]
            items[at] = (t[0], t[1], t[2], proofs[at % 8][(t[1] + 2) % 128])
        out.append(("two adjacent", items))
        items = list(good)
        mid = (n + 1) // 2      # the root [0, n) is split at ceil(n / 2)
        for at in {0, mid - 1, mid, n - 1}:
            t = items[at]
            items[at] = (t[0], t[1], CL.flip_low_bit(t[2], at % 64), t[3])
        out.append(("both sides of the root's split point", items))
    out.append(("everything false", [(t[0], t[1], t[2], proofs[i % 8][(t[1] + 1) % 128]) for i, t in enumerate(good)]))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 257])
def test_built_batches(hip, oracle, material, n):
    seen = set()
    for what, items in _defects(material, n):
        want = _expected(hip, oracle, items)
        stats = _check(_run(hip, items), want, (n, what))
        assert all(w[1] == 0 for w in want)
        f = want.count((False, 0))
        if what == "good":
            assert f == 0 and stats == [1, 0, 1]
        else:
            assert f >= 1, (n, what)
        if what == "everything false":
            assert f == n
        else:
            assert stats[1] == 0, (n, what, stats)
        seen.add(f)
    assert 1 in seen and (n == 1 or max(seen) == n)


# ---- invalid items ----

def _invalid_kinds(t):
    c, x, k, q = t
    assert GP.classify(CL.NOT_G1) == GP.NOT_IN_G1
    return [("index 128", (c, 128, k, q)), ("first element not canonical", (c, x, CL.non_canonical(k, 0), q)),
            ("last element not canonical", (c, x, CL.non_canonical(k, 63), q)), ("commitment outside G1", (CL.NOT_G1, x, k, q)),
            ("proof outside G1", (c, x, k, CL.NOT_G1))]


def test_invalid_items_at_wave_edges(hip, material):
    n = 130
    good = _good(material, n)
    lanes = (0, 63, 64, n - 1)
    for kind in range(5):
        items = list(good)
        for at in lanes:
            what, items[at] = _invalid_kinds(good[at])[kind]
        ret, ok, st, stats = _raw(hip, items)
        assert ret == BADARGS, what
        assert st == [1 if i in lanes else 0 for i in range(n)], what
        assert ok == [i not in lanes for i in range(n)], what
        assert stats == [1, 0, 1], (what, stats)
    # every kind in one batch, then nothing but invalid items
    items = list(good)
    for j, at in enumerate((0, 63, 64, 65, n - 1)):
        items[at] = _invalid_kinds(good[at])[j][1]
    ret, ok, st, stats = _raw(hip, items)
    assert ret == BADARGS and stats == [1, 0, 1] and ok == [s == 0 for s in st] and sum(st) == 5
    only = [_invalid_kinds(good[i])[i % 5][1] for i in range(70)]
    assert _raw(hip, only) == (BADARGS, [False] * 70, [1] * 70, [0, 0, 1])


def test_index_far_out_of_range(hip, material):
    good = _good(material, 3)
    for idx in (129, 255, 256, 2 ** 32, 2 ** 32 + 5, 2 ** 64 - 1):
        items = [good[0], (good[1][0], idx, good[1][2], good[1][3]), good[2]]
        assert _raw(hip, items) == (BADARGS, [True, False, True], [0, 1, 0], [1, 0, 1]), idx


# ---- repeats ----

def test_repeated_commitments_and_repeated_items(hip, oracle, material):
    a, b = _item(material, 2, 9), _item(material, 5, 9)
    items = [a, b, a, a, _item(material, 2, 10), b] + [_item(material, 2, c) for c in range(40)]
    want = [(True, 0)] * len(items)
    assert [CL.verdict(oracle, t) for t in items[:6]] == want[:6]
    assert _check(_run(hip, items), want) == [1, 0, 1]
    # the second copy of a repeated item spoilt: only that copy is false
    items[2] = (a[0], a[1], a[2], b[3])
    want[2] = CL.verdict(oracle, items[2])
    assert want[2] == (False, 0)
    _check(_run(hip, items), want)


# ---- hand-over ----

@pytest.mark.parametrize("opt", [0, 4])
def test_hand_over_to_the_per_lane_check(hip, material, opt):
    n = 257
    cm, cells, proofs = material
    items = _good(material, n)
    for at in (0, 1, 100, 128, 129, 256):
        t = items[at]
        items[at] = (t[0], t[1], t[2], proofs[at % 8][(t[1] + 1) % 128])
    items[200] = _invalid_kinds(items[200])[4][1]
    want = _groups_of_one(hip, items)
    assert want.count((False, 0)) == 6 and want.count((False, BADARGS)) == 1
    f = hip.lib.ckzg_hip_set_option
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_int64]
    ret0, ok0, st0, stats0 = _raw(hip, items)
    assert (ret0, list(zip(ok0, st0))) == (BADARGS, want) and stats0[1] == 0
    try:
        assert f(b"locate_max_checks", opt) == 0
        ret, ok, st, stats = _raw(hip, items)
    finally:
        assert f(b"locate_max_checks", 1024) == 0
    assert (ret, ok, st) == (ret0, ok0, st0)
    assert stats[0] <= max(opt, 1) and stats[1] > 0 and stats[2] == 1, stats


# ---- chunk edge ----

@pytest.mark.parametrize("at_second", [False, True])
def test_chunk_edge(hip, material, at_second):
    chunk = _chunk_cells()
    n = chunk + 1
    base = _good(material, 128)
    items = [base[i % 128] for i in range(n)]
    at = chunk if at_second else chunk - 1
    t = items[at]
    items[at] = (t[0], t[1], CL.flip_low_bit(t[2], 5), t[3])
    ok, st, stats = _run(hip, items)
    assert st == [0] * n and ok == [i != at for i in range(n)]
    assert stats[2] == 2 and stats[1] == 0
    if at_second:
        assert stats[0] == 2   # the first chunk's root check, and the second chunk's: one item, the check itself
    else:
        assert 3 <= stats[0] <= 2 + 2 * CL.ceil_log2(chunk)


# ---- two replicas ----

def test_shard_split_over_two_replicas(hip, material):
    # (two table replicas on one GPU stand in for two devices: the same fan-out, and no second GPU is needed)
    cm, cells, proofs = material
    items = _good(material, 300)
    for at in (0, 149, 150, 299):
        t = items[at]
        items[at] = (t[0], t[1], t[2], proofs[at % 8][(t[1] + 1) % 128])
    items[77] = _invalid_kinds(items[77])[0][1]
    want = _groups_of_one(hip, items)
    assert want.count((False, 0)) == 4 and want.count((False, BADARGS)) == 1
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        stats = _check(_run(api, items), want)
        assert stats[2] == 2 and stats[1] == 0
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


# ---- a forgery that equal weights would let through ----

def test_cancelling_forgery(hip, oracle, material):
    """two good cells of one column, proof_a + D and proof_b - D, D = [k]G: under equal weights the two errors cancel in
    both sums of the check.  Both must come out false, every other item true."""
    cm, cells, proofs = material
    rnd = random.Random(7594)
    d = GP.mul(GP.G, rnd.randrange(1, CL.R))
    for n, i, j in ((2, 0, 1), (70, 1, 64), (258, 1, 257)):
        items = _good(material, n)
        col = items[i][1]
        items[j] = _item(material, (j + 3) % 8, col)
        assert items[i][:3] != items[j][:3] and items[i][1] == items[j][1]
        pa, pb = GP.uncompress(items[i][3])[1], GP.uncompress(items[j][3])[1]
        items[i] = items[i][:3] + (GP.compress(GP.add(pa, d)),)
        items[j] = items[j][:3] + (GP.compress(GP.add(pb, GP.neg(d))),)
        assert CL.verdict(oracle, items[i]) == (False, 0) and CL.verdict(oracle, items[j]) == (False, 0)
        ok, st, stats = _run(hip, items)
        assert st == [0] * n and ok == [k not in (i, j) for k in range(n)], (n, i, j)


# ---- empty and NULL ----

def test_empty_call_and_null_arguments(hip, material):
    assert _run(hip, []) == ([], [], [0, 0, 0])
    f = getattr(hip.lib, NAME)
    f.restype = C.c_int
    assert f(None, None, None, None, None, None, None, C.c_uint64(0), hip.sp) == 0
    items = _good(material, 5)
    items[3] = (items[3][0], items[3][1], items[3][2], items[2][3])
    ret, ok, st, stats = _raw(hip, items, with_status=False, with_stats=False)
    assert (ret, ok, st, stats) == (0, [True, True, True, False, True], [7] * 5, [9, 9, 9])
    # NULL ok with n > 0: C_KZG_BADARGS, nothing written
    assert _raw(hip, items, with_ok=False) == (BADARGS, [True] * 5, [7] * 5, [9, 9, 9])
