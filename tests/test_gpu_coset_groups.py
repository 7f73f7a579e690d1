"""ckzg_hip_verify_coset_kzg_proof_batch_groups: ckzg_hip_verify_coset_kzg_proof_batch over many groups in one call, one
verdict per group, at every coset size 2^e.  Every group must come out exactly as the single call on its slice does, and
as its construction says: valid material comes from ckzg_hip_compute_coset_kzg_proofs_batch on two blobs
(tests/test_gpu_coset_openings.py pins that call) and stays valid however often it is repeated; a bumped value, a swapped
proof, a coset off by one or the other blob's commitment makes a group false.  Anchors outside the library: the CPU
oracle's verify_cell_kzg_proof_batch at e = 6, verify_kzg_proof at e = 0.  No expected value comes from the new call."""
import ctypes as C
import importlib.util
import os
import random
import re
import threading

import pytest

import g1_points as GP
from kzg_ctypes import HIP_SO, Kzg, KzgError
from test_gpu_coset_openings import EXT
from test_gpu_coset_verify import ES, R, _bump, _m, call, mat  # noqa: F401  (mat: the cached openings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARGS = 0, 1
NAME = "ckzg_hip_verify_coset_kzg_proof_batch_groups"
NOT_G1 = GP.by_label("Q+T11").data
NEW_KERNELS = ("k_coset_group_rlc_scalars", "k_coset_group_aggregate", "k_coset_group_interp", "k_coset_group_interp_sum")


def _chunk_items():
    src = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    return int(re.search(r"#define CKZG_HIP_COSET_GROUPS_CHUNK_ITEMS\s+(\d+)", src).group(1))


def _lists(items):
    """(commitment, coset, values, proof) items -> the four lists of the binding"""
    return tuple([it[k] for it in items] for k in range(4))


def _groups_call(api, groups, e):
    return api.verify_coset_kzg_proof_batch_groups([_lists(g) for g in groups], e)


def _check(got, expected):
    ok, st = got
    assert len(ok) == len(expected) and len(st) == len(expected)
    for g, exp in enumerate(expected):
        what = (g, ok[g], st[g], exp)
        if exp is None:
            assert st[g] == BADARGS and ok[g] is False, what
        else:
            assert st[g] == 0 and ok[g] is exp, what


def _with(item, cm=None, c=None, ev=None, pf=None):
    return (item[0] if cm is None else cm, item[1] if c is None else c, item[2] if ev is None else ev,
            item[3] if pf is None else pf)


def _mixed_groups(mat, e, seed):
    """about twenty groups of 0, 1, 2, 3 and 9 items of both blobs -- cosets 0, 1 and m - 1 among them, repeated items,
    cosets shared between groups -- true, false and invalid ones interleaved; (groups, expected)"""
    rnd = random.Random(seed)
    m, l = _m(e), 1 << e

    def honest(n):
        cs = [rnd.choice((0, 1, m - 1, rnd.randrange(m))) for _ in range(n)]
        return [mat.item(rnd.randrange(2), e, c) for c in cs]

    def spoil(n, how):
        g = honest(n)
        i = rnd.randrange(n)
        cm, c, ev, pf = g[i]
        b = 0 if cm == mat.commit[0] else 1
        if how == "value":
            g[i] = _bump(g[i], rnd.randrange(l), rnd.randrange(1, R))
        elif how == "proof":     # the proof of the next coset
            g[i] = _with(g[i], pf=mat.item(b, e, (c + 1) % m)[3])
        elif how == "coset":
            g[i] = _with(g[i], c=(c + 1) % m)
        elif how == "commitment":
            g[i] = _with(g[i], cm=mat.commit[1 - b])
        elif how == "proof not in G1":
            g[i] = _with(g[i], pf=NOT_G1)
        elif how == "commitment not in G1":
            g[i] = _with(g[i], cm=NOT_G1)
        elif how == "index = m":
            g[i] = _with(g[i], c=m)
        elif how == "value = r":
            j = rnd.randrange(l)
            g[i] = _with(g[i], ev=ev[:32 * j] + R.to_bytes(32, "big") + ev[32 * j + 32:])
        else:
            raise AssertionError(how)
        return g

    plan = [(9, None), (1, "value"), (0, None), (3, "proof not in G1"), (2, None), (9, "coset"), (1, None),
            (2, "commitment not in G1"), (3, None), (3, "commitment"), (9, "commitment not in G1"), (0, None), (9, None),
            (2, "proof"), (1, "index = m"), (3, None), (9, "value = r"), (1, "commitment not in G1"), (2, "value"), (9, None),
            (1, "proof")]
    groups, exp = [], []
    for n, how in plan:
        groups.append(spoil(n, how) if how else honest(n))
        exp.append(True if how is None else False if how in ("value", "proof", "coset", "commitment") else None)
    assert (exp.count(True), exp.count(False), exp.count(None)) == (9, 6, 6)
    return groups, exp


@pytest.mark.gpu
@pytest.mark.parametrize("e", ES)
def test_every_group_equals_the_single_call_on_its_slice(hip, mat, e):
    groups, exp = _mixed_groups(mat, e, 300 + e)
    single = [call(hip, g, e) for g in groups]
    assert single == [(BADARGS, False) if x is None else (OK, x) for x in exp]
    _check(_groups_call(hip, groups, e), exp)
    # ... in the opposite order too, and every group alone (the single-batch path of a one-group call)
    _check(_groups_call(hip, groups[::-1], e), exp[::-1])
    for g, x in zip(groups, exp):
        _check(_groups_call(hip, [g], e), [x])


@pytest.mark.gpu
def test_size_64_is_the_oracle_and_the_cell_groups_call(hip, oracle, mat):
    groups, exp = _mixed_groups(mat, 6, 640)
    want = []
    for g in groups:
        try:
            want.append(oracle.verify_cell_kzg_proof_batch(*_lists(g)))
        except KzgError:
            want.append(None)
    assert want == exp
    cells = hip.verify_cell_kzg_proof_batch_groups([_lists(g) for g in groups])
    _check(cells, exp)
    assert _groups_call(hip, groups, 6) == cells


@pytest.mark.gpu
def test_index_128_marks_its_own_group_at_the_cell_entry_and_at_the_coset_entry(hip, oracle, mat):
    """one pipeline behind both entries at e = 6, each with a range check of its own: three groups in one chunk, the
    middle one with index 128"""
    e, m = 6, _m(6)
    assert m == 128
    groups = [[mat.item(b, e, c) for c in (0, 5) for b in (0, 1)], [mat.item(0, e, 9), mat.item(1, e, 9), mat.item(0, e, 127)],
              [mat.item(1, e, 127)]]
    assert [oracle.verify_cell_kzg_proof_batch(*_lists(g)) for g in groups] == [True, True, True]
    _check(_groups_call(hip, groups, e), [True, True, True])
    groups[1][1] = _with(groups[1][1], c=m)
    exp = [True, None, True]
    with pytest.raises(KzgError):
        oracle.verify_cell_kzg_proof_batch(*_lists(groups[1]))
    assert call(hip, groups[1], e) == (BADARGS, False)
    _check(hip.verify_cell_kzg_proof_batch_groups([_lists(g) for g in groups]), exp)
    _check(_groups_call(hip, groups, e), exp)


@pytest.mark.gpu
def test_size_one_is_verify_kzg_proof(hip, mat):
    groups, exp = _mixed_groups(mat, 0, 100)
    valid = [(g, x) for g, x in zip(groups, exp) if x is not None]
    each = [all(hip.verify_kzg_proof(cm, EXT[c], y, pf) for cm, c, y, pf in g) for g, _ in valid]
    assert each == [x for _, x in valid]
    _check(_groups_call(hip, [g for g, _ in valid], 0), each)


# ---- soundness ----

def _forged(proof48):
    """(pi + D, pi - D), compressed: the cancelling pair of tests/test_gpu_coset_verify_soundness.py"""
    st, pi = GP.uncompress(proof48)
    assert st == 0 and pi is not GP.INF
    return GP.compress(GP.add(pi, GP.G)), GP.compress(GP.add(pi, GP.neg(GP.G)))


@pytest.mark.gpu
@pytest.mark.parametrize("e", ES)
def test_cancelling_forgeries_within_and_across_groups(hip, mat, e):
    rnd = random.Random(500 + e)
    m = _m(e)
    a = [mat.item(rnd.randrange(2), e, rnd.randrange(m)) for _ in range(9)]
    b = [mat.item(rnd.randrange(2), e, rnd.randrange(m)) for _ in range(5)]
    third = [mat.item(rnd.randrange(2), e, rnd.randrange(m)) for _ in range(3)]
    a[6] = a[2]
    b[2] = a[2]          # at the same offset of its group as a[2]: equal weights if the groups shared their randomness
    _check(_groups_call(hip, [a, b, third], e), [True, True, True])
    plus, minus = _forged(a[2][3])
    # both halves in one group
    fa = list(a)
    fa[2], fa[6] = _with(a[2], pf=plus), _with(a[2], pf=minus)
    _check(_groups_call(hip, [fa, b, third], e), [False, True, True])
    # one half in each of two groups
    fa, fb = list(a), list(b)
    fa[2], fb[2] = _with(a[2], pf=plus), _with(a[2], pf=minus)
    _check(_groups_call(hip, [fa, fb, third], e), [False, False, True])


# ---- cutting ----

def _swap_proofs(g, i, j):
    assert g[i][3] != g[j][3]
    g[i], g[j] = _with(g[i], pf=g[j][3]), _with(g[j], pf=g[i][3])


@pytest.mark.gpu
def test_chunk_boundary_inside_the_call_and_a_group_larger_than_a_chunk(hip, mat):
    e, chunk, per = 0, _chunk_items(), 512
    base = [mat.item(i % 2, e, (37 * i) % 8192) for i in range(64)]
    # groups of 512 repeated items: the call is cut after chunk / 512 groups; a wrong group on either side of the cut
    n = chunk // per + 8
    assert n * per > chunk > 4 * per
    groups = [[base[(g + i) % 64] for i in range(per)] for g in range(n)]
    exp = [True] * n
    for g in (chunk // per - 1, chunk // per, n - 1):
        _swap_proofs(groups[g], 5, 6)
        exp[g] = False
    groups[1][7] = _with(groups[1][7], cm=NOT_G1)
    exp[1] = None
    _check(_groups_call(hip, groups, e), exp)
    # one group larger than a chunk between two small ones, valid and then with two proofs swapped past the boundary
    big = [base[i % 64] for i in range(chunk + 64)]
    small = [base[:8], [_bump(base[8])] + base[9:16]]
    _check(_groups_call(hip, [small[0], big, small[1]], e), [True, True, False])
    _swap_proofs(big, chunk, chunk + 1)
    _check(_groups_call(hip, [small[0], big, small[1]], e), [True, False, False])


@pytest.mark.gpu
def test_4096_groups_of_one_item(hip, mat):
    e = 2
    rnd = random.Random(11)
    groups, exp = [], []
    for _ in range(4096):
        b, c, kind = rnd.randrange(2), rnd.randrange(64), rnd.randrange(8)
        it = mat.item(b, e, c)
        if kind == 0:
            it = _with(it, pf=mat.item(1 - b, e, c)[3])   # the other blob's proof for this coset
        elif kind == 1:
            it = _with(it, pf=NOT_G1)
        groups.append([it])
        exp.append(False if kind == 0 else None if kind == 1 else True)
    _check(_groups_call(hip, groups, e), exp)


# ---- fan-out and concurrency ----

def _some(mat, e, seed, n):
    rnd = random.Random(seed)
    groups, exp = [], []
    for _ in range(n):
        g = [mat.item(rnd.randrange(2), e, rnd.randrange(_m(e))) for _ in range(1 + rnd.randrange(8))]
        kind = rnd.randrange(4)
        if kind == 1:
            g[0] = _bump(g[0])
        elif kind == 2:
            g[-1] = _with(g[-1], cm=NOT_G1)
        groups.append(g)
        exp.append(False if kind == 1 else None if kind == 2 else True)
    return groups, exp


@pytest.mark.gpu
def test_groups_split_over_two_replicas(mat):
    # (two table replicas on one GPU stand in for two devices: the same fan-out, and no second GPU is needed)
    sets = [(e,) + _some(mat, e, 21 + e, 200) for e in (0, 3, 6)]
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        for e, groups, exp in sets:
            _check(_groups_call(api, groups, e), exp)
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


@pytest.mark.gpu
def test_concurrent_callers(hip, mat):
    sets = [(t % 7,) + _some(mat, t % 7, 100 + t, 20 + 15 * t) for t in range(8)]
    results, errors = [None] * 8, []

    def work(t):
        try:
            results[t] = _groups_call(hip, sets[t][1], sets[t][0])
        except Exception as ex:   # reported below
            errors.append(ex)

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors
    for t in range(8):
        _check(results[t], sets[t][2])


# ---- edges ----

def _raw_call(api, groups, e, with_status=True, start=None):
    g = len(groups)
    flat = [[it[k] for grp in groups for it in grp] for k in range(4)]
    if start is None:
        start = [0]
        for grp in groups:
            start.append(start[-1] + len(grp))
    ok = (C.c_bool * max(g, 1))(*([True] * max(g, 1)))
    st = (C.c_uint8 * max(g, 1))(*([7] * max(g, 1)))
    f = getattr(api.lib, NAME)
    f.restype = C.c_int
    ret = f(ok, st if with_status else None, b"".join(flat[0]), (C.c_uint64 * max(len(flat[1]), 1))(*flat[1]), b"".join(flat[2]),
            b"".join(flat[3]), (C.c_uint64 * len(start))(*start), C.c_uint64(g), C.c_uint32(e), api.sp)
    return ret, [bool(v) for v in ok[:g]], [int(v) for v in st[:g]]


@pytest.mark.gpu
def test_edges_of_the_argument_list(hip, mat):
    e = 3
    f = getattr(hip.lib, NAME)
    f.restype = C.c_int
    assert f(None, None, None, None, None, None, None, C.c_uint64(0), C.c_uint32(e), hip.sp) == 0
    assert hip.verify_coset_kzg_proof_batch_groups([], e) == ([], [])
    assert _groups_call(hip, [[]] * 5, e) == ([True] * 5, [0] * 5)
    groups = [[mat.item(b, e, 8 * g + i) for i in range(8) for b in (0, 1)][:8] for g in range(6)]
    groups[2][0] = _with(groups[2][0], pf=groups[2][2][3])   # a wrong proof
    groups[4][3] = _with(groups[4][3], c=_m(e))              # an index out of range
    exp = [True, True, False, True, None, True]
    ret, ok, st = _raw_call(hip, groups, e)
    assert ret == BADARGS
    _check((ok, st), exp)
    # status may be NULL
    ret2, ok2, st2 = _raw_call(hip, groups, e, with_status=False)
    assert (ret2, ok2, st2) == (BADARGS, ok, [7] * 6)
    ret3, ok3, _ = _raw_call(hip, groups[:4], e, with_status=False)
    assert (ret3, ok3) == (0, [True, True, False, True])
    # a malformed group_start: C_KZG_BADARGS, and nothing is written
    for start in ([1, 8, 16, 24, 32, 40, 48], [0, 8, 16, 15, 32, 40, 48]):
        assert _raw_call(hip, groups, e, start=start) == (BADARGS, [True] * 6, [7] * 6)
    # no such coset size: C_KZG_BADARGS, nothing is written, and the binding raises
    assert _raw_call(hip, groups[:2], 7) == (BADARGS, [True] * 2, [7] * 2)
    assert f(None, None, None, None, None, None, None, C.c_uint64(0), C.c_uint32(7), hip.sp) == BADARGS
    with pytest.raises(KzgError):
        hip.verify_coset_kzg_proof_batch_groups([], 7)
    # NULL ok or inputs with work to do
    start = (C.c_uint64 * 2)(0, 1)
    assert f(None, None, bytes(48), (C.c_uint64 * 1)(0), bytes(32 << e), bytes(48), start, C.c_uint64(1), C.c_uint32(e), hip.sp) == BADARGS
    ok1 = (C.c_bool * 1)(True)
    assert f(ok1, None, None, (C.c_uint64 * 1)(0), bytes(32 << e), bytes(48), start, C.c_uint64(1), C.c_uint32(e), hip.sp) == BADARGS
    assert ok1[0] is True


# ---- kernel resources ----

def test_coset_group_kernels_use_no_scratch():
    if os.environ.get("CKZG_HIP_SO"):
        pytest.skip("sanitizer / variant build: the budget is the product's")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    table = {k.split(":", 1)[1]: v for k, v in m.collect().items()}
    for name in NEW_KERNELS:
        assert name in table, name
        assert table[name]["scratch"] == 0, (name, table[name])
        assert table[name]["vgpr"] <= 128, (name, table[name])   # four waves per SIMD: short, latency-bound kernels
