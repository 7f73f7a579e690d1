"""ckzg_hip_verify_coset_kzg_proof_batch_locate: one ckzg_hip_verify_coset_kzg_proof_batch verdict per item, at every
coset size 2^e, e = 0 .. 6, at the cost of one batch check when every item verifies.  The proofs and values come from
ckzg_hip_compute_coset_kzg_proofs_batch, which tests/test_gpu_coset_openings.py pins at every size.  Expected verdicts
never come from the call under test: at every e from the existing ckzg_hip_verify_coset_kzg_proof_batch on the item
alone (once per distinct item), cross-checked at e = 0 against verify_kzg_proof and at e = 6 against the CPU oracle's
verify_cell_kzg_proof_batch and against ckzg_hip_verify_cell_kzg_proof_batch_locate on the same items."""
import ctypes as C
import random

import pytest

import cell_locate_items as CL
import coset_locate_expect as X
import g1_points as GP
from kzg_ctypes import HIP_SO, Kzg
from test_gpu_coset_openings import EXT
from test_gpu_coset_verify import Material, _bump, call as verify_call

pytestmark = pytest.mark.gpu
NAME = "ckzg_hip_verify_coset_kzg_proof_batch_locate"
BADARGS = X.BADARGS
R = X.R
ES = list(range(7))


def _m(e):
    return 8192 >> e


@pytest.fixture(scope="module")
def mat(hip):
    return Material(hip)


def _good(mat, e, n):
    """n good items: blob i mod 2, coset 7 i + 3 mod m"""
    return [mat.item(i % 2, e, (7 * i + 3) % _m(e)) for i in range(n)]


def _run(api, items, e):
    return api.verify_coset_kzg_proof_batch_locate(*[[t[k] for t in items] for k in range(4)], e)


def _raw(api, items, e, with_status=True, with_stats=True, with_ok=True):
    n = len(items)
    f = getattr(api.lib, NAME)
    f.restype = C.c_int
    ok = (C.c_bool * max(n, 1))(*([True] * max(n, 1)))
    st = (C.c_uint8 * max(n, 1))(*([7] * max(n, 1)))
    stats = (C.c_uint64 * 3)(9, 9, 9)
    j = lambda k: b"".join(t[k] for t in items)
    ret = f(ok if with_ok else None, st if with_status else None, stats if with_stats else None, j(0),
            (C.c_uint64 * max(n, 1))(*[t[1] for t in items]), j(2), j(3), C.c_uint64(n), C.c_uint32(e), api.sp)
    return ret, [bool(v) for v in ok[:n]], [int(v) for v in st[:n]], [int(v) for v in stats]


_ALONE = {}


def _alone(hip, item, e):
    """(ok, status) of the existing batch call on the one item; one call per distinct item"""
    key = (e,) + tuple(item)
    if key not in _ALONE:
        ret, ok = verify_call(hip, [item], e)
        assert ret in (0, BADARGS) and not (ret and ok)
        _ALONE[key] = (ok, ret)
    return _ALONE[key]


def _expected(hip, items, e):
    return [_alone(hip, t, e) for t in items]


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
        assert 1 <= stats[0] <= stats[2] - 1 + X.checks_bound(f, n), (what, stats)
    return stats


# ---- built batches ----

def _defects(mat, e, n):
    """(what, items): the good batch of n with defects of each kind"""
    good = _good(mat, e, n)
    m, l = _m(e), 1 << e
    p = n // 2
    cm, c, ev, pf = good[p]
    b = p % 2
    out = [("good", good)]

    def one(what, item, at=p):
        items = list(good)
        items[at] = item
        out.append((what, items))

    one("first value bumped", _bump(good[p], 0))
    one("last value bumped", _bump(good[p], l - 1))
    one("proof of another item", (cm, c, ev, mat.item(b, e, (c + 1) % m)[3]))
    one("the other commitment", (mat.commit[1 - b], c, ev, pf))
    one("coset off by one", (cm, (c + 1) % m, ev, pf))
    if n >= 2:
        items = list(good)
        for at in (p - 1, p):
            t = items[at]
            items[at] = (t[0], t[1], t[2], mat.item(at % 2, e, (t[1] + 2) % m)[3])
        out.append(("two adjacent", items))
        items = list(good)
        mid = (n + 1) // 2      # the root [0, n) is split at ceil(n / 2)
        for at in {0, mid - 1, mid, n - 1}:
            items[at] = _bump(items[at], at % l, 1 + at)
        out.append(("both sides of the root's split point", items))
    out.append(("everything false", [(t[0], t[1], t[2], mat.item(i % 2, e, (t[1] + 1) % m)[3]) for i, t in enumerate(good)]))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 257])
@pytest.mark.parametrize("e", ES)
def test_built_batches(hip, mat, e, n):
    seen = set()
    for what, items in _defects(mat, e, n):
        want = _expected(hip, items, e)
        stats = _check(_run(hip, items, e), want, (e, n, what))
        assert all(w[1] == 0 for w in want)
        f = want.count((False, 0))
        if what == "good":
            assert f == 0 and stats == [1, 0, 1]
        else:
            assert f >= 1, (e, n, what)
        if what == "everything false":
            assert f == n
        else:
            assert stats[1] == 0, (e, n, what, stats)
        seen.add(f)
    assert 1 in seen and (n == 1 or max(seen) == n)


# ---- anchors outside the library's coset verifier ----

def test_size_one_against_verify_kzg_proof(hip, mat):
    cs = [0, 1, 4095, 4096, 8191] + random.Random(8).sample(range(8192), 11)
    items = [mat.item(b, 0, c) for c in cs for b in (0, 1)]
    items[9] = _bump(items[9])
    items[20] = (items[20][0], items[20][1], items[20][2], items[21][3])
    each = [hip.verify_kzg_proof(cm, EXT[c], y, pf) for cm, c, y, pf in items]
    assert each == [i not in (9, 20) for i in range(len(items))]
    assert [w[0] for w in _expected(hip, items, 0)] == each
    ok, st, stats = _run(hip, items, 0)
    assert ok == each and st == [0] * len(items)


def test_size_64_against_the_oracle_and_the_cell_form(hip, oracle, mat):
    items = _good(mat, 6, 70)
    items[33] = _bump(items[33], 63)
    items[34] = (items[34][0], items[34][1], items[34][2], items[35][3])
    items[50] = (items[50][0], 128, items[50][2], items[50][3])
    items[51] = (items[51][0], items[51][1], CL.non_canonical(items[51][2], 63), items[51][3])
    items[52] = (CL.NOT_G1, items[52][1], items[52][2], items[52][3])
    want = [CL.verdict(oracle, t) for t in items]
    assert want.count((False, 0)) == 2 and want.count((False, BADARGS)) == 3
    assert _expected(hip, items, 6) == want
    ret, ok, st, stats = _raw(hip, items, 6)
    assert ret == BADARGS and list(zip(ok, st)) == want
    ok2, st2, stats2 = hip.verify_cell_kzg_proof_batch_locate(*[[t[k] for t in items] for k in range(4)])
    assert (ok, st) == (ok2, st2) and stats == stats2


# ---- repeats ----

@pytest.mark.parametrize("e", ES)
def test_repeated_commitments_and_repeated_items(hip, mat, e):
    a, b = mat.item(0, e, 9), mat.item(1, e, 9)
    items = [a, b, a, a, mat.item(0, e, 10), b] + [mat.item(0, e, c) for c in range(40)]
    want = [(True, 0)] * len(items)
    assert _expected(hip, items[:6], e) == want[:6]
    assert _check(_run(hip, items, e), want) == [1, 0, 1]
    items[2] = (a[0], a[1], a[2], b[3])   # the second copy of a repeated item spoilt: only that copy is false
    want[2] = _alone(hip, items[2], e)
    assert want[2] == (False, 0)
    _check(_run(hip, items, e), want)


# ---- invalid items ----

def _invalid_kinds(t, e):
    cm, c, ev, pf = t
    l = 1 << e
    r32 = R.to_bytes(32, "big")
    on_curve_not_g1 = CL.NOT_G1
    off_curve = next(bytes([0x80]) + x.to_bytes(47, "big") for x in range(1, 200)
                     if GP.classify(bytes([0x80]) + x.to_bytes(47, "big")) == GP.BAD_ENCODING)
    assert GP.classify(on_curve_not_g1) == GP.NOT_IN_G1
    return [("index m", (cm, _m(e), ev, pf)), ("first value r", (cm, c, r32 + ev[32:], pf)),
            ("last value r", (cm, c, ev[:32 * (l - 1)] + r32, pf)), ("commitment off the curve", (off_curve, c, ev, pf)),
            ("proof off the curve", (cm, c, ev, off_curve)), ("commitment outside the subgroup", (on_curve_not_g1, c, ev, pf)),
            ("proof outside the subgroup", (cm, c, ev, on_curve_not_g1))]


@pytest.mark.parametrize("e", ES)
def test_invalid_items_in_a_good_batch(hip, mat, e):
    n = 130
    good = _good(mat, e, n)
    lanes = (0, 63, 64, n - 1)
    for kind in range(7):
        items = list(good)
        for at in lanes:
            what, items[at] = _invalid_kinds(good[at], e)[kind]
        assert _alone(hip, items[63], e) == (False, BADARGS), what
        ret, ok, st, stats = _raw(hip, items, e)
        assert ret == BADARGS, what
        assert st == [1 if i in lanes else 0 for i in range(n)], what
        assert ok == [i not in lanes for i in range(n)], what
        assert stats == [1, 0, 1], (what, stats)
    only = [_invalid_kinds(good[i], e)[i % 7][1] for i in range(70)]
    assert _raw(hip, only, e) == (BADARGS, [False] * 70, [1] * 70, [0, 0, 1])
    for idx in (_m(e) + 1, 2 ** 32, 2 ** 32 + 5, 2 ** 64 - 1):
        items = [good[0], (good[1][0], idx, good[1][2], good[1][3]), good[2]]
        assert _raw(hip, items, e) == (BADARGS, [True, False, True], [0, 1, 0], [1, 0, 1]), idx


# ---- hand-over ----

@pytest.mark.parametrize("opt", [0, 4])
@pytest.mark.parametrize("e", [0, 3, 6])
def test_hand_over_to_the_per_lane_check(hip, mat, e, opt):
    n = 257
    items = _good(mat, e, n)
    for at in (0, 1, 100, 128, 129, 256):
        t = items[at]
        items[at] = (t[0], t[1], t[2], mat.item(at % 2, e, (t[1] + 1) % _m(e))[3])
    items[200] = _invalid_kinds(items[200], e)[6][1]
    want = _expected(hip, items, e)
    assert want.count((False, 0)) == 6 and want.count((False, BADARGS)) == 1
    f = hip.lib.ckzg_hip_set_option
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_int64]
    ret0, ok0, st0, stats0 = _raw(hip, items, e)
    assert (ret0, list(zip(ok0, st0))) == (BADARGS, want) and stats0[1] == 0
    try:
        assert f(b"locate_max_checks", opt) == 0
        ret, ok, st, stats = _raw(hip, items, e)
    finally:
        assert f(b"locate_max_checks", 1024) == 0
    assert (ret, ok, st) == (ret0, ok0, st0)
    assert stats[0] <= max(opt, 1) and stats[1] > 0 and stats[2] == 1, stats


# ---- chunk edge ----

@pytest.mark.parametrize("at_second", [False, True])
@pytest.mark.parametrize("e", [0, 3, 6])
def test_chunk_edge(hip, mat, e, at_second):
    chunk = X.chunk_items(e)
    n = chunk + 1
    base = _good(mat, e, 128)
    assert _expected(hip, base, e) == [(True, 0)] * 128
    items = [base[i % 128] for i in range(n)]
    at = chunk if at_second else chunk - 1
    items[at] = _bump(items[at], (1 << e) - 1)
    assert _alone(hip, items[at], e) == (False, 0)
    ok, st, stats = _run(hip, items, e)
    assert st == [0] * n and ok == [i != at for i in range(n)]
    assert stats[2] == 2 and stats[1] == 0
    if at_second:
        assert stats[0] == 2   # the first chunk's root check, and the second chunk's: one item, the check itself
    else:
        assert 3 <= stats[0] <= 2 + 2 * X.ceil_log2(chunk)


# ---- two replicas ----

@pytest.mark.parametrize("e", [1, 6])
def test_shard_split_over_two_replicas(hip, mat, e):
    # (two table replicas on one GPU stand in for two devices: the same fan-out, and no second GPU is needed)
    items = _good(mat, e, 300)
    for at in (0, 149, 150, 299):
        t = items[at]
        items[at] = (t[0], t[1], t[2], mat.item(at % 2, e, (t[1] + 1) % _m(e))[3])
    items[77] = _invalid_kinds(items[77], e)[0][1]
    want = _expected(hip, items, e)
    assert want.count((False, 0)) == 4 and want.count((False, BADARGS)) == 1
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        stats = _check(_run(api, items, e), want)
        assert stats[2] == 2 and stats[1] == 0
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


# ---- a forgery that equal weights would let through ----

@pytest.mark.parametrize("e", [0, 3, 6])
def test_cancelling_forgery(hip, mat, e):
    """two good items on one coset, proof_a + D and proof_b - D, D = [k]G: under equal weights the two errors cancel in
    both sums of the check.  Both must come out false, every other item true."""
    rnd = random.Random(7594 + e)
    d = GP.mul(GP.G, rnd.randrange(1, R))
    for n, i, j in ((2, 0, 1), (70, 1, 64), (258, 1, 257)):
        items = _good(mat, e, n)
        c = items[i][1]
        items[j] = mat.item(1 - i % 2, e, c)
        assert items[i][:3] != items[j][:3] and items[i][1] == items[j][1]
        pa, pb = GP.uncompress(items[i][3])[1], GP.uncompress(items[j][3])[1]
        items[i] = items[i][:3] + (GP.compress(GP.add(pa, d)),)
        items[j] = items[j][:3] + (GP.compress(GP.add(pb, GP.neg(d))),)
        assert _alone(hip, items[i], e) == (False, 0) and _alone(hip, items[j], e) == (False, 0)
        ok, st, stats = _run(hip, items, e)
        assert st == [0] * n and ok == [k not in (i, j) for k in range(n)], (e, n, i, j)


# ---- empty, NULL, a size out of range ----

def test_empty_call_and_null_arguments(hip, mat):
    f = getattr(hip.lib, NAME)
    f.restype = C.c_int
    for e in ES:
        assert _run(hip, [], e) == ([], [], [0, 0, 0])
        assert f(None, None, None, None, None, None, None, C.c_uint64(0), C.c_uint32(e), hip.sp) == 0
    e = 2
    items = _good(mat, e, 5)
    items[3] = (items[3][0], items[3][1], items[3][2], items[2][3])
    ret, ok, st, stats = _raw(hip, items, e, with_status=False, with_stats=False)
    assert (ret, ok, st, stats) == (0, [True, True, True, False, True], [7] * 5, [9, 9, 9])
    # NULL ok with n > 0, or a coset size past 64: C_KZG_BADARGS, nothing written
    assert _raw(hip, items, e, with_ok=False) == (BADARGS, [True] * 5, [7] * 5, [9, 9, 9])
    big = [(t[0], t[1], t[2] * 16, t[3]) for t in items]
    assert _raw(hip, big, 7) == (BADARGS, [True] * 5, [7] * 5, [9, 9, 9])
