"""ckzg_hip_g1_prefix_sums, ckzg_hip_verify_kzg_proof_batch_locate and ckzg_hip_verify_blob_kzg_proof_batch_locate
(c-kzg-4844_amd/csrc/locate.hip, locate_plan.hpp): prefix sums against the oracle's additions, compared as points; every
item's verdict against the consensus vectors, the CPU oracle or the library's per-item call -- never against the call
under test; the counts in `stats` as the rules of the bisection fix them; the hand-over to the per-lane check; the chunk
edge; the blob form."""
import ctypes as C
import hashlib
import os
import random
import re

import pytest

from conftest import ORACLE_SO, ROOT
from golden_util import case_names, get_case
from kzg_ctypes import HIP_SO, Kzg
from test_gpu_point_proofs import INF, R, _fr, _spec_items

pytestmark = pytest.mark.gpu
BADARGS = 1
TILE = 256          # locate.hip: SCAN_TILE
CHUNK = 65536       # ckzg_hip.h: CKZG_HIP_LOCATE_CHUNK_ITEMS
G48 = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")


# ---- prefix sums ----

class G1:
    """g1_t values (144 bytes, Jacobian) and their arithmetic through the oracle"""

    def __init__(self):
        self.o = o = C.CDLL(ORACLE_SO)
        o.og1_equal.restype = C.c_bool
        aff = C.create_string_buffer(96)
        assert o.og1_uncompress(aff, G48) == 0
        gen = C.create_string_buffer(144)
        o.og1_from_affine(gen, aff)
        self.gen, self.inf = gen.raw, bytes(144)

    def add(self, a, b):
        r = C.create_string_buffer(144)
        self.o.og1_add(r, a, b)
        return r.raw

    def neg(self, a):
        r = C.create_string_buffer(144)
        self.o.og1_neg(r, a)
        return r.raw

    def mul(self, a, k):
        r = C.create_string_buffer(144)
        self.o.og1_mul_raw(r, a, (C.c_uint64 * 4)(*[(k >> (64 * i)) & (2 ** 64 - 1) for i in range(4)]), 255)
        return r.raw

    def eq(self, a, b):
        return bool(self.o.og1_equal(a, b))


@pytest.fixture(scope="module")
def g1():
    return G1()


@pytest.fixture(scope="module")
def pool(g1):
    """200 distinct points with random (not unit) Z, and what the oracle says their multiples of G are"""
    rnd = random.Random(11)
    pts = []
    for _ in range(200):
        k = rnd.randrange(1, R)
        # k G as (k - j) G + j G: the oracle's addition leaves a Z that is not one
        j = rnd.randrange(1, R)
        pts.append(g1.add(g1.mul(g1.gen, (k - j) % R), g1.mul(g1.gen, j)))
    return pts


def _inputs(g1, pool, n, seed, identity_at):
    """n points: the identity at the first and last index and at identity_at; a run P, P (doubling); P, -P followed by
    more points"""
    rnd = random.Random(seed)
    p = [pool[rnd.randrange(len(pool))] for _ in range(n)]
    for i in identity_at:
        if 0 <= i < n:
            p[i] = g1.inf
    if n >= 8:
        p[2] = p[1] = pool[5]                        # running sum after index 1 is P (index 0 is the identity): P + P
        p[4], p[5] = pool[9], g1.neg(pool[9])        # P, -P, then more points
    if n >= 600:                                     # the same across a tile boundary
        p[TILE - 1], p[TILE] = pool[3], g1.neg(pool[3])
        p[2 * TILE - 1] = p[2 * TILE] = pool[4]
    if n:
        p[0] = p[n - 1] = g1.inf
    return p


def _check_prefix(g1, hip, p):
    out = hip.g1_prefix_sums(p)
    assert len(out) == len(p)
    acc = g1.inf
    for i, q in enumerate(p):
        acc = g1.add(acc, q)
        assert g1.eq(out[i], acc), i
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_prefix_sums_small(hip, g1, pool, n):
    bounds = [b for b in range(TILE, n, TILE)] + [64]
    _check_prefix(g1, hip, _inputs(g1, pool, n, n, []))
    _check_prefix(g1, hip, _inputs(g1, pool, n, n + 1, [b - 1 for b in bounds] + bounds))   # identity on both sides of every boundary
    _check_prefix(g1, hip, [g1.inf] * n)
    if n >= 2:   # -P right after P at the very start, and P alone doubled
        _check_prefix(g1, hip, [pool[0], g1.neg(pool[0])] + [pool[1]] * (n - 2))
        _check_prefix(g1, hip, [pool[0]] * n)


@pytest.mark.parametrize("n", [TILE * TILE - 1, TILE * TILE, TILE * TILE + 1])
def test_prefix_sums_around_the_second_level(hip, g1, pool, n):
    """65,535 / 65,536 / 65,537 points: below, at and above tile^2, where the totals level recurses.  Identity on both
    sides of every second tile boundary and of the tile^2 boundary."""
    bounds = [b for b in range(TILE, n, TILE) if (b // TILE) % 2 == 1] + [TILE * TILE]
    p = _inputs(g1, pool, n, n, [b - 1 for b in bounds] + bounds)
    out = _check_prefix(g1, hip, p)   # every prefix against the oracle's running sum ...
    # ... and, independently of a running sum: the total from the multiplicities, and out[i] - out[i - 1] == p[i]
    count = {}
    for q in p:
        count[q] = count.get(q, 0) + 1
    total = g1.inf
    for q, c in count.items():
        total = g1.add(total, g1.mul(q, c))
    assert g1.eq(out[n - 1], total)
    rnd = random.Random(n)
    idx = {i for b in range(TILE, n, TILE) for i in (b - 1, b, b + 1) if i < n} | {rnd.randrange(1, n) for _ in range(1000)}
    for i in sorted(idx):
        assert g1.eq(g1.add(out[i], g1.neg(out[i - 1])), p[i]), i


def test_all_identity_at_the_second_level(hip, g1):
    n = TILE * TILE + 1
    out = hip.g1_prefix_sums([g1.inf] * n)
    assert all(q[96:144] == bytes(48) for q in out)   # Z = 0


# ---- point form ----

def _run(api, items):
    return api.verify_kzg_proof_batch_locate([t[0] for t in items], [t[1] for t in items], [t[2] for t in items],
                                             [t[3] for t in items])


def _check(got, items):
    ok, st, stats = got
    assert len(ok) == len(items) and len(st) == len(items) and len(stats) == 3
    for i, it in enumerate(items):
        exp = it[4]
        if exp is None:
            assert st[i] == BADARGS and ok[i] is False, (i, it[5:])
        else:
            assert st[i] == 0 and ok[i] is exp, (i, it[5:], ok[i], exp)
    return stats


def _ceil_log2(m):
    return (m - 1).bit_length()


def _bound(items, chunks=1):
    nfalse = sum(1 for t in items if t[4] is False)
    return chunks + 2 * nfalse * _ceil_log2(min(len(items), CHUNK))


def test_all_spec_vectors_in_one_call(hip):
    items = _spec_items()
    assert len(items) >= 100 and {t[4] for t in items} == {True, False, None}
    stats = _check(_run(hip, items), items)
    assert 1 < stats[0] <= _bound(items) and stats[2] == 1


def test_special_vectors_at_wave_edges(hip):
    items = _spec_items()
    is_special = lambda t: t[4] is not True or t[0] == INF or t[3] == INF
    special = [t for t in items if is_special(t)]
    plain = [t for t in items if not is_special(t)]
    assert special and plain and {t[4] for t in special} == {True, False, None}
    rnd = random.Random(3)
    for n in (1, 2, 3, 5, 64, 65, 257):
        batch = [plain[rnd.randrange(len(plain))] for _ in range(n)]
        for j, lane in enumerate(sorted({0, 1, 31, 32, 63, 64, 65, n - 1})):
            if lane < n:
                batch[lane] = special[(j + n) % len(special)]
        stats = _check(_run(hip, batch), batch)
        assert stats[0] <= _bound(batch), (n, stats)


@pytest.fixture(scope="module")
def tuples(hip):
    """64 valid (commitment, z, y, proof) from the library's compute_kzg_proof on random blobs, checked by the oracle in
    `checked`; a quarter of the z on the evaluation domain"""
    rnd = random.Random(7)
    w = pow(7, (R - 1) // 4096, R)
    out = []
    for i in range(64):
        blob = b"".join(_fr(rnd.randrange(R)) for _ in range(4096))
        c = hip.blob_to_kzg_commitment(blob)
        z = _fr(pow(w, rnd.randrange(4096), R)) if i % 4 == 0 else _fr(rnd.randrange(R))
        proof, y = hip.compute_kzg_proof(blob, z)
        out.append((c, z, y, proof))
    return out


@pytest.fixture(scope="module")
def checked(tuples, oracle):
    for t in tuples:
        assert _oracle_verdict(oracle, t) is True
    return [t + (True, "good") for t in tuples]


def _wrong_y(t):
    return (t[0], t[1], _fr(int.from_bytes(t[2], "big") + 1), t[3], False, "wrong y")


def _built(checked, n, kind):
    """n items from the checked tuples with the named defect; expected verdicts are by construction for 'wrong y' (the
    evaluation is unique) and confirmed by the caller's reference for the rest"""
    items = [checked[i % len(checked)] for i in range(n)]
    mid = (n + 1) // 2   # the root's split point
    if kind == "wrong y":
        items[n // 3] = _wrong_y(items[n // 3])
    elif kind == "wrong proof":
        i = n // 3
        items[i] = items[i][:3] + (checked[(i + 1) % len(checked)][3], False, "another proof")
    elif kind == "swapped commitment":
        i = n - 1
        items[i] = (checked[(i + 1) % len(checked)][0],) + items[i][1:4] + (False, "another commitment")
    elif kind == "adjacent":
        items[n // 2] = _wrong_y(items[n // 2])
        if n > 1:
            items[n // 2 - 1] = _wrong_y(items[n // 2 - 1])
    elif kind == "both sides":
        items[mid - 1] = _wrong_y(items[mid - 1])
        if mid < n:
            items[mid] = _wrong_y(items[mid])
    elif kind == "all":
        items = [_wrong_y(t) for t in items]
    return items


_ORACLE_VERDICTS = {}


def _oracle_verdict(oracle, t):
    """the oracle's verify_kzg_proof, computed once per distinct item"""
    if t not in _ORACLE_VERDICTS:
        _ORACLE_VERDICTS[t] = oracle.verify_kzg_proof(*t)
    return _ORACLE_VERDICTS[t]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 257])
def test_built_items(hip, oracle, checked, n):
    for kind in ("wrong y", "wrong proof", "swapped commitment", "adjacent", "both sides", "all"):
        items = _built(checked, n, kind)
        # the expected verdicts: the oracle per item (n <= 65), the library's per-item call otherwise
        if n <= 65:
            ref = [_oracle_verdict(oracle, t[:4]) for t in items]
        else:
            ref, st = hip.verify_kzg_proof_batch([t[0] for t in items], [t[1] for t in items], [t[2] for t in items], [t[3] for t in items])
            assert st == [0] * n
        assert ref == [t[4] for t in items], kind
        assert not all(ref)
        stats = _check(_run(hip, items), items)
        if kind != "all":
            assert stats[0] <= _bound(items) and stats[1] == 0, (kind, n, stats)


def test_stats_all_good_one_false_one_invalid(hip, checked):
    n = 257
    good = [checked[i % 64] for i in range(n)]
    assert _check(_run(hip, good), good) == [1, 0, 1]
    one = list(good)
    one[200] = _wrong_y(one[200])
    stats = _check(_run(hip, one), one)
    assert 1 < stats[0] <= 1 + 2 * 9 and stats[1] == 0 and stats[2] == 1
    inv = list(good)
    inv[77] = (inv[77][0], R.to_bytes(32, "big")) + inv[77][2:4] + (None, "z not canonical")
    assert _check(_run(hip, inv), inv) == [1, 0, 1]   # an invalid item alone triggers no bisection
    allinv = [inv[77]] * 3
    assert _check(_run(hip, allinv), allinv) == [0, 0, 1]   # no valid item: no check


def test_hand_over_to_the_per_lane_check(hip, checked):
    n = 257
    items = [checked[i % 64] for i in range(n)]
    for i in (3, 100, 101, 128, 129, 256):
        items[i] = _wrong_y(items[i])
    items[50] = (items[50][0], items[50][1], R.to_bytes(32, "big"), items[50][3], None, "y not canonical")
    free = _check(_run(hip, items), items)
    assert free[1] == 0
    f = hip.lib.ckzg_hip_set_option
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_int64]
    try:
        for opt in (0, 4):
            assert f(b"locate_max_checks", opt) == 0
            stats = _check(_run(hip, items), items)   # identical verdicts
            assert stats[0] <= max(opt, 1) and stats[1] > 0 and stats[2] == 1, (opt, stats)   # (the root check is always run)
            good = [checked[i % 64] for i in range(n)]
            assert _check(_run(hip, good), good) == [1, 0, 1]
    finally:
        assert f(b"locate_max_checks", DEFAULT_MAX_CHECKS) == 0


def _default_max_checks():
    src = open(os.path.join(ROOT, "c-kzg-4844_amd", "csrc", "ckzg_api.hip")).read()
    return int(re.search(r"g_locate_max_checks\{(\d+)\}", src).group(1))


DEFAULT_MAX_CHECKS = _default_max_checks()


def test_empty_call_and_null_arguments(hip, checked):
    assert _run(hip, []) == ([], [], [0, 0, 0])
    f = hip.lib.ckzg_hip_verify_kzg_proof_batch_locate
    f.restype = C.c_int
    assert f(None, None, None, None, None, None, None, C.c_uint64(0), hip.sp) == 0
    items = [checked[0], _wrong_y(checked[1]), checked[2]]
    j = lambda k: b"".join(t[k] for t in items)
    ok = (C.c_bool * 3)()
    assert f(ok, None, None, j(0), j(1), j(2), j(3), C.c_uint64(3), hip.sp) == 0   # status and stats may be NULL
    assert list(ok) == [True, False, True]
    assert f(None, None, None, j(0), j(1), j(2), j(3), C.c_uint64(3), hip.sp) == BADARGS


@pytest.mark.parametrize("at", [CHUNK - 1, CHUNK])
def test_chunk_edge(hip, checked, at):
    """65,537 items made by repeating the 64 checked ones, one false item on either side of the chunk boundary"""
    n = CHUNK + 1
    items = [checked[i % 64] for i in range(n)]
    items[at] = _wrong_y(items[at])
    ok, st, stats = _run(hip, items)
    assert st == [0] * n and ok == [i != at for i in range(n)]
    assert stats[2] == 2 and stats[1] == 0
    if at == CHUNK:   # alone in the second chunk: that chunk's root check is the item's own check
        assert stats[0] == 2
    else:
        assert 2 < stats[0] <= 2 + 2 * 16


def test_shard_split_over_two_replicas(checked):
    items = [checked[i % 64] for i in range(300)]
    for i in (0, 149, 150, 299):
        items[i] = _wrong_y(items[i])
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        stats = _check(_run(api, items), items)
        assert stats[2] == 2 and stats[0] <= 2 + 2 * 4 * 8
    finally:
        api.close()
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


# ---- blob form ----

def _check_blobs(got, expected, names=None):
    ok, st, stats = got
    assert len(ok) == len(expected) and len(st) == len(expected)
    for i, exp in enumerate(expected):
        what = (i, names[i] if names else None, ok[i], st[i], exp)
        if exp is None:
            assert st[i] == BADARGS and ok[i] is False, what
        else:
            assert st[i] == 0 and ok[i] is exp, what
    return stats


def test_all_blob_spec_vectors_in_one_call(hip):
    blobs, cms, proofs, exp, names = [], [], [], [], []
    for name in case_names("verify_blob_kzg_proof"):
        inp, e = get_case("verify_blob_kzg_proof", name)
        b, c, p = inp["blob"], inp["commitment"], inp["proof"]
        if any(v is None for v in (b, c, p)) or len(b) != 131072 or len(c) != 48 or len(p) != 48:
            continue
        blobs.append(b), cms.append(c), proofs.append(p), exp.append(e), names.append(name)
    assert len(exp) >= 20 and set(exp) == {True, False, None}
    stats = _check_blobs(hip.verify_blob_kzg_proof_batch_locate(blobs, cms, proofs), exp, names)
    assert stats[2] == 1 and 1 < stats[0] <= 1 + 2 * exp.count(False) * _ceil_log2(len(exp))


@pytest.fixture(scope="module")
def material(oracle):
    """5 blobs with their commitments and blob proofs from the CPU oracle"""
    blobs = [b"".join(b"\x00" + hashlib.sha256(b"locate%d/%d" % (i, j)).digest()[:31] for j in range(4096)) for i in range(5)]
    cms = [oracle.blob_to_kzg_commitment(b) for b in blobs]
    return blobs, cms, [oracle.compute_blob_kzg_proof(b, c) for b, c in zip(blobs, cms)]


def _blob_cases(material, n):
    blobs, cms, proofs = (list(v[:n]) for v in material)
    yield "good", blobs, cms, proofs
    yield "wrong proof", blobs, cms, proofs[:n - 1] + [material[2][(n - 1 + 1) % 5]]
    yield "commitment of another blob", blobs, [material[1][(0 + 1) % 5]] + cms[1:], proofs
    bad = bytearray(blobs[n // 2])
    bad[32 * 7:32 * 8] = R.to_bytes(32, "big")   # a non-canonical field element
    yield "non-canonical element", blobs[:n // 2] + [bytes(bad)] + blobs[n // 2 + 1:], cms, proofs


def _oracle_blob(oracle, b, c, p):
    try:
        return oracle.verify_blob_kzg_proof(b, c, p)
    except Exception:
        return None


@pytest.mark.parametrize("n", [1, 2, 5])
def test_built_blobs_against_the_oracle(hip, oracle, material, n):
    seen = set()
    for what, blobs, cms, proofs in _blob_cases(material, n):
        exp = [_oracle_blob(oracle, b, c, p) for b, c, p in zip(blobs, cms, proofs)]
        seen |= set(exp)
        stats = _check_blobs(hip.verify_blob_kzg_proof_batch_locate(blobs, cms, proofs), exp, [what] * n)
        nvalid = sum(1 for e in exp if e is not None)
        assert stats[2] == 1 and stats[0] <= (1 if nvalid else 0) + 2 * exp.count(False) * _ceil_log2(n), (what, stats)
        if all(e is True for e in exp):
            assert stats[:2] == [1, 0]
    assert seen == {True, False, None}


def test_blobs_split_over_two_replicas(oracle, material):
    blobs, cms, proofs = (list(v) for v in material)
    proofs[3] = material[2][0]
    exp = [_oracle_blob(oracle, b, c, p) for b, c, p in zip(blobs, cms, proofs)]
    assert exp == [True, True, True, False, True]
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        stats = _check_blobs(api.verify_blob_kzg_proof_batch_locate(blobs, cms, proofs), exp)
        assert stats[2] == 2
    finally:
        api.close()
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)
