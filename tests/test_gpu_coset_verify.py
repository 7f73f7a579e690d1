"""ckzg_hip_verify_coset_kzg_proof_batch: the verdicts, at every coset size 2^e, e = 0 .. 6 (c-kzg-4844_amd/csrc/
coset_verify.hip; the model is tests/coset_verify_expect.py).  The proofs and values come from
ckzg_hip_compute_coset_kzg_proofs_batch, which tests/test_gpu_coset_openings.py pins at every size.  The reference is
never the call under test: e = 6 hangs on the oracle's verify_cell_kzg_proof_batch (the library's is the same pipeline at
e = 6, and must agree with both), e = 0 on verify_kzg_proof,
e = 1 .. 5 on a single-item check by definition in the oracle's group arithmetic on the setup file's points."""
import ctypes as C
import random

import pytest

import coset_verify_expect as V
import domain_expect as D
import g1_points
from conftest import SHIM_SO
from kzg_ctypes import HIP_SO, TRUSTED_SETUP, Kzg
from test_gpu_coset_openings import EXT, INF48, Levels, _jac
from test_gpu_locate import G1
from test_gpu_point_openings import _blob, _fr

pytestmark = pytest.mark.gpu
R = D.R
OK, BADARGS = 0, 1
ES = list(range(7))


def _m(e):
    return 8192 >> e


@pytest.fixture(scope="module")
def g1():
    return G1()


@pytest.fixture(scope="module")
def constants():
    what = (C.c_uint64 * 6)()
    C.CDLL(SHIM_SO).hs_coset_verify_constants(what)
    return dict(zip(("per_lane", "max_parts", "hash_on_pool_from", "min_shard", "agg_slots", "interp_threads"), what))


class Material:
    """two blobs, their commitments and, per (blob, e), the proofs and values of one compute call"""

    def __init__(self, hip):
        self.hip = hip
        self.blobs = [_blob(0xC05E + i) for i in range(2)]
        self.commit = [hip.blob_to_kzg_commitment(b) for b in self.blobs]
        self.levels = Levels(hip)

    def item(self, b, e, c):
        proofs, evals = self.levels(self.blobs[b], e)
        per = 32 << e
        return (self.commit[b], c, evals[per * c:per * (c + 1)], proofs[c])

    def mixed(self, e, seed):
        """cosets 0, 1, m - 1 and a handful of random ones of both blobs, interleaved"""
        m = _m(e)
        cs = [0, 1, m - 1] + random.Random(seed).sample(range(2, m - 1), min(6, m - 3))
        return [self.item(b, e, c) for c in cs for b in (0, 1)]


@pytest.fixture(scope="module")
def mat(hip):
    return Material(hip)


def call(api, items, e):
    """(return value, verdict) of the call on (commitment, coset, values, proof) items"""
    n = len(items)
    f = api._fn("ckzg_hip_verify_coset_kzg_proof_batch")
    ok = C.c_bool(True)
    ret = f(C.byref(ok), b"".join(i[0] for i in items), (C.c_uint64 * max(n, 1))(*[i[1] for i in items]),
            b"".join(i[2] for i in items), b"".join(i[3] for i in items), C.c_uint64(n), C.c_uint32(e), api.sp)
    return ret, ok.value


def _ints(ev):
    return [int.from_bytes(ev[32 * j:32 * j + 32], "big") for j in range(len(ev) // 32)]


def _bump(item, j=0, delta=1):
    cm, c, ev, pf = item
    ys = _ints(ev)
    ys[j] = (ys[j] + delta) % R
    return (cm, c, b"".join(_fr(y) for y in ys), pf)


# ---- true batches ----

@pytest.mark.parametrize("e", ES)
def test_true_batches(hip, mat, e):
    one = mat.item(0, e, 5 % _m(e))
    assert call(hip, [one], e) == (OK, True)
    mixed = mat.mixed(e, 40 + e)
    assert len({i[0] for i in mixed}) == 2
    assert call(hip, mixed, e) == (OK, True)
    assert call(hip, [one, one], e) == (OK, True)
    assert call(hip, [mat.item(0, e, 3), mat.item(1, e, 3)], e) == (OK, True)
    # ... and through the binding
    assert hip.verify_coset_kzg_proof_batch([i[0] for i in mixed], [i[1] for i in mixed], [i[2] for i in mixed],
                                            [i[3] for i in mixed], e) is True


@pytest.mark.parametrize("e", ES)
def test_one_false_item_anywhere(hip, mat, e):
    mixed = mat.mixed(e, 60 + e)
    l = 1 << e
    for pos in (0, len(mixed) // 2, len(mixed) - 1):
        for j in sorted({0, l - 1}):
            bad = mixed[:pos] + [_bump(mixed[pos], j)] + mixed[pos + 1:]
            assert call(hip, bad, e) == (OK, False), (pos, j)
    cm, c, ev, pf = mixed[2]
    assert call(hip, mixed[:2] + [(cm, c, ev, mixed[3][3])] + mixed[3:], e) == (OK, False)      # another item's proof
    assert call(hip, mixed[:2] + [(mixed[3][0], c, ev, pf)] + mixed[3:], e) == (OK, False)      # the other commitment
    assert call(hip, mixed[:2] + [(cm, (c + 1) % _m(e), ev, pf)] + mixed[3:], e) == (OK, False)  # the coset off by one


# ---- anchors ----

def test_size_64_is_verify_cell_kzg_proof_batch(hip, oracle, mat):
    items = [mat.item(0, 6, c) for c in range(128)]
    for batch, want in ((items, True), (items[:77] + [_bump(items[77], 63)] + items[78:], False)):
        args = ([i[0] for i in batch], [i[1] for i in batch], [i[2] for i in batch], [i[3] for i in batch])
        assert hip.verify_cell_kzg_proof_batch(*args) is want
        assert oracle.verify_cell_kzg_proof_batch(*args) is want
        assert call(hip, batch, 6) == (OK, want)


def test_size_one_is_verify_kzg_proof(hip, mat):
    cs = [0, 1, 4095, 4096, 8191] + random.Random(8).sample(range(8192), 11)
    items = [mat.item(b, 0, c) for c in cs for b in (0, 1)]
    forged = items[:9] + [_bump(items[9])] + items[10:]
    for batch, false_at in ((items, None), (forged, 9)):
        each = [hip.verify_kzg_proof(cm, EXT[c], y, pf) for cm, c, y, pf in batch]
        assert each == [i != false_at for i in range(len(batch))]
        assert call(hip, batch, 0) == (OK, all(each))
        for i, it in enumerate(batch):
            if i in (0, 9, len(batch) - 1):
                assert call(hip, [it], 0) == (OK, each[i])


# ---- by definition, independent of the library ----

class Setup:
    """the setup file's points through the oracle: g1_values_monomial[0 .. 31], g2_values_monomial[0 .. 64]"""

    def __init__(self, g1):
        lines = open(TRUSTED_SETUP).read().split()
        assert (int(lines[0]), int(lines[1])) == (4096, 65)
        self.g1 = g1
        self.mono = [_jac(g1, bytes.fromhex(h)) for h in lines[2 + 4096 + 65:2 + 4096 + 65 + 32]]
        self.g2 = []
        for h in lines[2 + 4096:2 + 4096 + 65]:
            aff, jac = C.create_string_buffer(192), C.create_string_buffer(288)
            assert g1.o.og2_uncompress(aff, bytes.fromhex(h)) == 0
            g1.o.og2_from_affine(jac, aff)
            self.g2.append(jac.raw)
        g1.o.opairings_verify.restype = C.c_bool

    def holds(self, item, e):
        """e(C - [I(s)]_1 + [x_c^l] pi, [1]_2) = e(pi, [s^l]_2)"""
        g1 = self.g1
        cm, c, ev, pf = item
        a = V.interp_coeffs(_ints(ev), c, e)
        i_s = g1.inf
        for ak, pt in zip(a, self.mono):
            i_s = g1.add(i_s, g1.mul(pt, ak))
        pi = _jac(g1, pf)
        xl = pow(D.root_of_unity(8192), V.shift_root(c, e), R)
        lhs = g1.add(g1.add(_jac(g1, cm), g1.neg(i_s)), g1.mul(pi, xl))
        return bool(g1.o.opairings_verify(lhs, self.g2[0], pi, self.g2[1 << e]))


@pytest.fixture(scope="module")
def setup(g1):
    return Setup(g1)


@pytest.mark.parametrize("e", range(1, 6))
def test_single_items_by_definition(hip, mat, setup, e):
    m = _m(e)
    c = random.Random(e).randrange(1, m - 1)
    true = mat.item(0, e, c)
    cm, _, ev, pf = true
    cases = [true,
             _bump(true, random.Random(e + 9).randrange(1 << e)),
             (cm, c, ev, mat.item(0, e, c + 1)[3]),      # the neighbouring coset's proof
             (cm, c + 1, ev, pf),                        # the coset index off by one
             (mat.commit[1], c, ev, pf)]                 # the other blob's commitment
    want = [setup.holds(it, e) for it in cases]
    assert want == [True, False, False, False, False]
    assert [call(hip, [it], e) for it in cases] == [(OK, w) for w in want]


# ---- soundness of the combination ----

@pytest.mark.parametrize("e", ES)
def test_errors_that_cancel_under_equal_weights_are_caught(hip, mat, e):
    """two items on one coset under one commitment, value j off by +delta in one and by -delta in the other: the sum of
    the two interpolation polynomials is right, so a combination with equal weights accepts the pair"""
    rnd = random.Random(300 + e)
    item = mat.item(1, e, rnd.randrange(_m(e)))
    j, delta = rnd.randrange(1 << e), rnd.randrange(1, R)
    assert call(hip, [item, item], e) == (OK, True)
    assert call(hip, [_bump(item, j, delta), _bump(item, j, R - delta)], e) == (OK, False)
    others = mat.mixed(e, 7)[:4]
    assert call(hip, others[:2] + [_bump(item, j, delta)] + others[2:] + [_bump(item, j, R - delta)], e) == (OK, False)


# ---- edges ----

@pytest.mark.parametrize("e", ES)
def test_zero_polynomial(hip, e):
    items = [(INF48, c, bytes(32 << e), INF48) for c in (0, 1, _m(e) - 1)]
    assert call(hip, items, e) == (OK, True)
    assert call(hip, items[:1], e) == (OK, True)
    assert call(hip, [_bump(items[1])] + items, e) == (OK, False)


@pytest.mark.parametrize("e", [0, 6])
def test_constant_polynomial(hip, e):
    k = 0x1234567
    cm = hip.blob_to_kzg_commitment(D.blob_of_poly([k]))
    items = [(cm, c, _fr(k) * (1 << e), INF48) for c in (0, 7, _m(e) - 1)]
    assert call(hip, items, e) == (OK, True)
    assert call(hip, items[:2] + [_bump(items[2], (1 << e) - 1)], e) == (OK, False)


def test_nothing_to_do(hip):
    for e in ES:
        assert call(hip, [], e) == (OK, True)
        f = hip._fn("ckzg_hip_verify_coset_kzg_proof_batch")
        ok = C.c_bool(False)
        assert f(C.byref(ok), None, None, None, None, C.c_uint64(0), C.c_uint32(e), hip.sp) == OK and ok.value


def _alone_and_amid(hip, mat, e, bad):
    true = mat.mixed(e, 90)[:6]
    assert call(hip, [bad], e) == (BADARGS, False)
    assert call(hip, true[:3] + [bad] + true[3:], e) == (BADARGS, False)


@pytest.mark.parametrize("e", ES)
def test_bad_arguments(hip, mat, e):
    true = mat.mixed(e, 91)[:6]
    cm, c, ev, pf = true[2]
    l, m = 1 << e, _m(e)
    assert call(hip, true, 7) == (BADARGS, False)
    for idx in (m, 8192, 2 ** 64 - 1):
        _alone_and_amid(hip, mat, e, (cm, idx, ev, pf))
    for j in sorted({0, l - 1}):      # a value equal to r
        _alone_and_amid(hip, mat, e, (cm, c, ev[:32 * j] + R.to_bytes(32, "big") + ev[32 * j + 32:], pf))
    f = hip._fn("ckzg_hip_verify_coset_kzg_proof_batch")
    idx1 = (C.c_uint64 * 1)(c)
    for args in ((None, idx1, ev, pf), (cm, None, ev, pf), (cm, idx1, None, pf), (cm, idx1, ev, None)):
        ok = C.c_bool(True)
        assert f(C.byref(ok), *args, C.c_uint64(1), C.c_uint32(e), hip.sp) == BADARGS and not ok.value
    assert call(hip, true, e) == (OK, True)


BAD_POINTS = [x for x in g1_points.corpus() if x.expected != g1_points.VALID]
BAD_LABELS = ["T3", "neg(T3)", "generic", "Q+T11", "no_compression_bit", "inf_with_x", "inf_with_sign", "x=p", "off_curve"]


@pytest.mark.parametrize("e", ES)
def test_invalid_points_in_either_slot(hip, mat, e):
    labels = {x.label for x in BAD_POINTS}
    classes = {x.expected for x in BAD_POINTS}
    chosen = [x for x in BAD_POINTS if x.label in BAD_LABELS]
    assert {x.expected for x in chosen} == classes and len(classes) == 2, labels
    cm, c, ev, pf = mat.item(0, e, 2)
    for x in chosen:
        _alone_and_amid(hip, mat, e, (x.data, c, ev, pf))
        _alone_and_amid(hip, mat, e, (cm, c, ev, x.data))


# ---- thresholds ----

def _repeat(mat, e, n, blob=0):
    m = _m(e)
    base = [mat.item(blob, e, c) for c in range(min(m, n))]
    return (base * (n // len(base) + 1))[:n]


@pytest.mark.parametrize("e", [0, 3, 6])
def test_transcript_on_the_worker_pool(hip, mat, constants, e):
    t = constants["hash_on_pool_from"]
    assert t > 1
    for n in (t - 1, t):
        items = _repeat(mat, e, n)
        assert call(hip, items, e) == (OK, True)
        assert call(hip, items[:-1] + [_bump(items[-1], (1 << e) - 1)], e) == (OK, False)


@pytest.mark.parametrize("e", [4, 6])
def test_aggregate_in_parts(hip, mat, constants, e):
    """the first size at which a column is split over two lanes, and the size below it; at e = 6 also four parts"""
    first = _m(e) * constants["per_lane"] + 1
    shim = C.CDLL(SHIM_SO)
    shim.hs_coset_verify_agg_parts.restype = C.c_uint32
    sizes = [first - 1, first] + ([2 * (first - 1), 2 * (first - 1) + 1] if e == 6 else [])
    assert [shim.hs_coset_verify_agg_parts(C.c_uint64(n), e) for n in sizes] == [1, 2, 2, 4][:len(sizes)]
    for n in sizes:
        items = _repeat(mat, e, n)
        assert call(hip, items, e) == (OK, True)
        assert call(hip, items[:n // 2] + [_bump(items[n // 2])] + items[n // 2 + 1:], e) == (OK, False)


CALL_TABLE_FROM = 128   # ckzg_api2.hip: verify_cosets_wants_table (CKZG_HIP_VERIFY_CELL_TABLE_MIN), at e = 6 only


@pytest.mark.parametrize("e,n", [(6, CALL_TABLE_FROM - 1), (6, CALL_TABLE_FROM), (5, CALL_TABLE_FROM)])
def test_call_time_table_threshold(hip, oracle, mat, setup, e, n):
    """cosets of 64 take their four sums from a call-time table from 128 items on (what verify_cell_kzg_proof_batch runs),
    from ladders below; smaller cosets from ladders at every size.  The verdicts are the CPU oracle's: its
    verify_cell_kzg_proof_batch at e = 6, the check of each item by definition at e = 5"""
    items = _repeat(mat, e, n)
    at = n - 2
    forged = items[:at] + [_bump(items[at], 1)] + items[at + 1:]
    if e == 6:
        for batch, want in ((items, True), (forged, False)):
            assert oracle.verify_cell_kzg_proof_batch(*[[it[k] for it in batch] for k in range(4)]) is want
    else:
        assert all(setup.holds(it, e) for it in items) and not setup.holds(forged[at], e)
    assert call(hip, items, e) == (OK, True)
    assert call(hip, forged, e) == (OK, False)


def test_every_point_of_the_domain_in_one_call(hip, mat):
    """e = 0, 8192 columns of one value with one item each; the sums take the one-lane ladders from here on"""
    items = [mat.item(1, 0, c) for c in range(8192)]
    assert call(hip, items, 0) == (OK, True)
    assert call(hip, items[:8191] + [_bump(items[8191])], 0) == (OK, False)


# ---- several devices ----

def test_split_over_two_replicas(mat, constants):
    # (two table replicas on one GPU stand in for two devices: the same fan-out, and no second GPU is needed)
    n = 2 * constants["min_shard"] + 5
    items = _repeat(mat, 2, n)
    at = n - 3                      # in the second shard
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        assert call(api, items, 2) == (OK, True)
        assert call(api, items[:at] + [_bump(items[at], 3)] + items[at + 1:], 2) == (OK, False)
        assert call(api, items[:at] + [(items[at][0], items[at][1], items[at][2], BAD_POINTS[0].data)] + items[at + 1:],
                    2) == (BADARGS, False)
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)
