"""Cancelling forgeries through ckzg_hip_verify_coset_kzg_proof_batch, at every coset size (the pattern of
tests/test_gpu_rlc_soundness.py).  The weights r^i of the batch check are the one value its
verdicts cannot check on honest or independently spoilt inputs.  Put the same honest item at positions i and j of a
batch and replace its proofs by pi + D and pi - D, D the generator -- or one of its values by y + d and y - d: the two
errors cancel in every sum of the check exactly when w_i = w_j (the coset, its factor x_c^l and the commitment are equal
because the items are; tests/test_coset_verify_expect_cpu.py shows the acceptance under equal weights in the model).  A
correct library rejects the batch; one whose weights collide at (i, j) accepts it.

No expected value comes from the call under test: the same batch with the forgery removed must be true, and at e = 6 the
CPU oracle's verify_cell_kzg_proof_batch says False for every forged batch.  The pairs are those of the neighbouring
file: (0, 1), (1, 64), (63, 129), (5, 255) and (1, 257), (2, 258), (1, 65) -- i = j modulo 256 or 64, what a power table
that drops a high bit of the index, or an exponent cut to a wave, would collide on -- in a batch of 260 items, which
also stands above the size from which the transcript is hashed on the worker pool."""
import random

import pytest

import g1_points as gp
from test_gpu_coset_verify import ES, OK, R, _bump, _m, call, mat  # noqa: F401  (mat: the cached openings)

pytestmark = pytest.mark.gpu
PAIRS = [(0, 1), (1, 64), (63, 129), (5, 255), (1, 257), (2, 258), (1, 65)]
N = 260


def _forged(proof48):
    """(pi + D, pi - D), compressed"""
    st, pi = gp.uncompress(proof48)
    assert st == 0 and pi is not gp.INF
    return gp.compress(gp.add(pi, gp.G)), gp.compress(gp.add(pi, gp.neg(gp.G)))


def _batch(mat, e, i, j, seed):
    """260 honest items of both blobs with the same item at i and j"""
    rnd = random.Random(seed)
    m = _m(e)
    items = [mat.item(rnd.randrange(2), e, rnd.randrange(m)) for _ in range(N)]
    items[j] = items[i]
    return items


@pytest.mark.parametrize("e", ES)
def test_forged_proof_pairs(hip, oracle, mat, e):
    for i, j in PAIRS:
        items = _batch(mat, e, i, j, 100 * e + i + j)
        assert call(hip, items, e) == (OK, True), (i, j)
        cm, c, ev, pf = items[i]
        plus, minus = _forged(pf)
        forged = list(items)
        forged[i], forged[j] = (cm, c, ev, plus), (cm, c, ev, minus)
        if e == 6 and (i, j) == PAIRS[0]:
            assert oracle.verify_cell_kzg_proof_batch(*[[it[k] for it in forged] for k in range(4)]) is False
        assert call(hip, forged, e) == (OK, False), (i, j)


@pytest.mark.parametrize("e", ES)
def test_forged_value_pairs(hip, mat, e):
    rnd = random.Random(900 + e)
    for i, j in PAIRS:
        items = _batch(mat, e, i, j, 200 * e + i + j)
        pos, delta = rnd.randrange(1 << e), rnd.randrange(1, R)
        forged = list(items)
        forged[i], forged[j] = _bump(items[i], pos, delta), _bump(items[i], pos, R - delta)
        assert call(hip, forged, e) == (OK, False), (i, j)


@pytest.mark.parametrize("i,j", [(0, 1), (63, 129), (1, 65)])
def test_forged_proof_pairs_over_the_call_time_table(hip, oracle, mat, i, j):
    """e = 6, 130 items: the scalars are rows of the table's matrix (from 128 items on), as verify_cell_kzg_proof_batch
    lays them out; both verdicts are the CPU oracle's"""
    items = _batch(mat, 6, i, j, 7000 + i + j)[:130]
    cm, c, ev, pf = items[i]
    plus, minus = _forged(pf)
    forged = list(items)
    forged[i], forged[j] = (cm, c, ev, plus), (cm, c, ev, minus)
    for batch, want in ((items, True), (forged, False)):
        assert oracle.verify_cell_kzg_proof_batch(*[[it[k] for it in batch] for k in range(4)]) is want
        assert call(hip, batch, 6) == (OK, want), (i, j)
