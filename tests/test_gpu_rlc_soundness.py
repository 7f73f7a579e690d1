"""Cancelling forgeries through every public entry point that batches.  The weights r^i of a batch check are the one
value its verdicts cannot check on honest or independently spoilt inputs; what wrong weights cost is soundness: two
errors that cancel under equal weights are accepted.  The construction is one fact.  Put the same honest item at
positions i and j of a batch and replace its proofs by pi + D and pi - D, D the generator: the two errors cancel in
both sums of the check exactly when w_i = w_j (z, the column's coset factor and the commitment are equal because the
items are).  A correct library rejects the batch; one whose weights collide at (i, j) -- r^(i mod 256), powers that
restart at a chunk edge, r = 1 -- accepts it.

No expected value comes from the library under test: the CPU oracle's batch function says False for every forged
batch and True for the same batch with D removed (both asserted), so the weights are the only reason to reject.

The shapes are the smallest that reach each path; they follow the thresholds of the code:
  * verify_blob_kzg_proof_batch: the host path is n <= SMALL_VERIFY_N = 3; the pipelined form starts at option
    verify_pipe_min (default 1024, set to 16 here) and moves chunks of 256 blobs, so the chunk-crossing pair is
    (1, 257) in a batch of 260.
  * verify_cell_kzg_proof_batch makes its scalars on the device from 128 cells on (the call-time table) and on the host
    below: n = 127 and 128 stand on both sides.
  * ckzg_hip_verify_blob_cell_kzg_proof_batch_groups derives the cells itself, blob by blob: equal items are the same
    column of two copies of a blob, so its pairs are (c, c + 128) and (c, c + 256).
  * next to the pairs (0, 1), (1, 64), (63, 129) and (5, 255) stand (1, 257), (2, 258) and (1, 65): i = j modulo 256
    or 64, what a power table that drops a high bit of the index, or an exponent cut to a wave, would collide on."""
import ctypes as C
import hashlib

import pytest

import g1_points as gp
from test_gpu_round3 import _device, rt  # noqa: F401  (rt: the HIP runtime fixture of the resident form)

pytestmark = pytest.mark.gpu
VERIFY_CHUNK = 256      # ckzg_api2.hip: piped_form, CH
CELL_TABLE_MIN = 128    # ckzg_api2.hip: verify_cosets_wants_table, table_min


def _forged(proof48):
    """(pi + D, pi - D), compressed"""
    st, pi = gp.uncompress(proof48)
    assert st == 0 and pi is not gp.INF
    return gp.compress(gp.add(pi, gp.G)), gp.compress(gp.add(pi, gp.neg(gp.G)))


def _with_pair(proofs, i, j, pair):
    out = list(proofs)
    out[i], out[j] = pair
    return out


class _Option:
    """a call-time option for the length of a with block"""

    def __init__(self, hip, key, value, default):
        self.f, self.key, self.value, self.default = hip.lib.ckzg_hip_set_option, key, value, default
        self.f.restype = C.c_int
        self.f.argtypes = [C.c_char_p, C.c_int64]

    def __enter__(self):
        assert self.f(self.key, self.value) == 0

    def __exit__(self, *exc):
        assert self.f(self.key, self.default) == 0


@pytest.fixture(scope="module")
def mat(oracle):
    """one honest blob with its commitment, blob proof, cells and cell proofs, and one honest point opening"""
    blob = b"".join(b"\x00" + hashlib.sha256(b"rlcsound/%d" % j).digest()[:31] for j in range(4096))
    cm = oracle.blob_to_kzg_commitment(blob)
    proof = oracle.compute_blob_kzg_proof(blob, cm)
    cells, cproofs = oracle.compute_cells_and_kzg_proofs(blob)
    z = (0x1234567 << 200).to_bytes(32, "big")
    pproof, y = oracle.compute_kzg_proof(blob, z)
    m = dict(blob=blob, cm=cm, proof=proof, cells=cells, cproofs=cproofs, z=z, y=y, pproof=pproof)
    assert oracle.verify_blob_kzg_proof(blob, cm, proof) and oracle.verify_kzg_proof(cm, z, y, pproof)
    m["blob_pair"] = _forged(proof)
    m["point_pair"] = _forged(pproof)
    for p in m["blob_pair"]:
        assert not oracle.verify_blob_kzg_proof(blob, cm, p)
    for p in m["point_pair"]:
        assert not oracle.verify_kzg_proof(cm, z, y, p)
    return m


# ---- verify_blob_kzg_proof_batch ----

_blob_oracle = {}


def _blob_batch(oracle, mat, n, i, j):
    """(blobs, commitments, forged proofs); the oracle's two verdicts asserted once per shape"""
    blobs, cms = [mat["blob"]] * n, [mat["cm"]] * n
    forged = _with_pair([mat["proof"]] * n, i, j, mat["blob_pair"])
    if (n, i, j) not in _blob_oracle:
        _blob_oracle[(n, i, j)] = (oracle.verify_blob_kzg_proof_batch(blobs, cms, forged),
                                   oracle.verify_blob_kzg_proof_batch(blobs, cms, [mat["proof"]] * n))
    assert _blob_oracle[(n, i, j)] == (False, True)
    return blobs, cms, forged


@pytest.mark.parametrize("n,i,j", [(2, 0, 1), (9, 0, 1), (9, 1, 2), (9, 3, 8)])
def test_blob_batch_rejects_a_cancelling_pair(hip, oracle, mat, rt, n, i, j):  # noqa: F811
    """n = 2: the host path (n <= SMALL_VERIFY_N); n = 9: the one-copy form with the call-time table (from 8 blobs);
    each with host and GPU challenge hashing, and the resident form"""
    blobs, cms, forged = _blob_batch(oracle, mat, n, i, j)
    assert hip.verify_blob_kzg_proof_batch(blobs, cms, [mat["proof"]] * n) is True
    assert hip.verify_blob_kzg_proof_batch(blobs, cms, forged) is False
    with _Option(hip, b"gpu_sha_min", 1, 0):
        assert hip.verify_blob_kzg_proof_batch(blobs, cms, forged) is False
    assert _device(hip, rt, b"".join(blobs), b"".join(cms), b"".join(forged), n) == (0, False)
    assert _device(hip, rt, b"".join(blobs), b"".join(cms), b"".join([mat["proof"]] * n), n) == (0, True)


def test_blob_batch_rejects_a_pair_at_equal_offsets_of_two_chunks(hip, oracle, mat, rt):  # noqa: F811
    """260 blobs, the pair at (1, 1 + 256): the pipelined form (verify_pipe_min lowered to 16; chunks of 256), where
    powers that restart per chunk would give both halves r^1; then the one-copy form with the challenges hashed on
    the GPU, and the resident form"""
    n, i, j = VERIFY_CHUNK + 4, 1, 1 + VERIFY_CHUNK
    blobs, cms, forged = _blob_batch(oracle, mat, n, i, j)
    with _Option(hip, b"verify_pipe_min", 16, 1024):
        assert hip.verify_blob_kzg_proof_batch(blobs, cms, [mat["proof"]] * n) is True
        assert hip.verify_blob_kzg_proof_batch(blobs, cms, forged) is False
        with _Option(hip, b"gpu_sha_min", 1, 0):
            assert hip.verify_blob_kzg_proof_batch(blobs, cms, forged) is False
    assert hip.verify_blob_kzg_proof_batch(blobs, cms, forged) is False      # default options: one copy
    assert _device(hip, rt, b"".join(blobs), b"".join(cms), b"".join(forged), n) == (0, False)


# ---- verify_cell_kzg_proof_batch ----

def _cell_items(mat, n, i, j):
    """n cells of the honest blob, columns 3 k mod 128, positions i and j the same (commitment, column, cell)"""
    cols = [(3 * k) % 128 for k in range(n)]
    cols[j] = cols[i]
    cells = [mat["cells"][c] for c in cols]
    honest = [mat["cproofs"][c] for c in cols]
    return [mat["cm"]] * n, cols, cells, honest, _with_pair(honest, i, j, _forged(honest[i]))


@pytest.mark.parametrize("n,i,j", [(2, 0, 1), (CELL_TABLE_MIN - 1, 1, 64), (CELL_TABLE_MIN, 1, 64), (130, 0, 1), (130, 63, 129),
                                   (260, 2, 258)])
def test_cell_batch_rejects_a_cancelling_pair(hip, oracle, mat, n, i, j):
    """the scalars are k_coset_rlc_scalars' at every size: below 128 cells as the vectors of the ladder sums, from 128 on
    as rows of the call-time table's matrix"""
    cms, cols, cells, honest, forged = _cell_items(mat, n, i, j)
    assert oracle.verify_cell_kzg_proof_batch(cms, cols, cells, honest) is True
    assert oracle.verify_cell_kzg_proof_batch(cms, cols, cells, forged) is False
    assert hip.verify_cell_kzg_proof_batch(cms, cols, cells, honest) is True
    assert hip.verify_cell_kzg_proof_batch(cms, cols, cells, forged) is False


# ---- the three _groups calls ----

# (size, forged pair or None): every forged group stands between honest ones, and each size has an honest twin
GROUP_SHAPES = [(2, None), (2, (0, 1)), (65, None), (65, (1, 64)), (130, None), (130, (63, 129)), (3, None), (66, (1, 65)),
                (66, None)]


def test_blob_groups_reject_exactly_the_forged_groups(hip, oracle, mat):
    """also two neighbouring groups with the forged halves at the same offset in each: each must fail on its own (one
    half per group is an error no weight can cancel; the pair only cancels if the groups' sums are merged)"""
    groups, want = [], []
    for size, pair in GROUP_SHAPES:
        proofs = [mat["proof"]] * size
        if pair:
            proofs = _with_pair(proofs, pair[0], pair[1], mat["blob_pair"])
        groups.append(([mat["blob"]] * size, [mat["cm"]] * size, proofs))
        want.append(pair is None)
    for half in mat["blob_pair"]:
        groups.append(([mat["blob"]] * 4, [mat["cm"]] * 4, _with_pair([mat["proof"]] * 4, 2, 2, (half, half))))
        want.append(False)
    groups.append(([mat["blob"]] * 4, [mat["cm"]] * 4, [mat["proof"]] * 4))
    want.append(True)
    assert [oracle.verify_blob_kzg_proof_batch(*g) for g in groups] == want
    ok, st = hip.verify_blob_kzg_proof_batch_groups(groups)
    assert st == [0] * len(groups) and ok == want


def test_cell_groups_reject_exactly_the_forged_groups(hip, oracle, mat):
    groups, want = [], []
    for size, pair in GROUP_SHAPES + [(260, (2, 258)), (260, None)]:
        i, j = pair if pair else (0, 0)
        cms, cols, cells, honest, forged = _cell_items(mat, size, i, j)
        groups.append((cms, cols, cells, forged if pair else honest))
        want.append(pair is None)
    half_p, half_m = _forged(mat["cproofs"][6])
    for half in (half_p, half_m):
        cms, cols, cells, honest, _ = _cell_items(mat, 4, 0, 0)
        assert cols[2] == 6
        groups.append((cms, cols, cells, honest[:2] + [half] + honest[3:]))
        want.append(False)
    assert [oracle.verify_cell_kzg_proof_batch(*g) for g in groups] == want
    ok, st = hip.verify_cell_kzg_proof_batch_groups(groups)
    assert st == [0] * len(groups) and ok == want


def test_blob_cell_groups_reject_exactly_the_forged_groups(hip, oracle, mat):
    """the call derives the cells itself, so the equal items are one column of two copies of the blob: pairs
    (c, c + 128) within two copies and (c, c + 256) within three"""
    def group(copies, pair):
        proofs = list(mat["cproofs"]) * copies
        if pair:
            proofs = _with_pair(proofs, pair[0], pair[1], _forged(proofs[pair[0]]))
        return ([mat["blob"]] * copies, [mat["cm"]] * copies, proofs)

    shapes = [(1, None), (2, (0, 128)), (2, None), (2, (63, 191)), (3, None), (3, (5, 261)), (1, None)]
    groups = [group(c, p) for c, p in shapes]
    want = [p is None for _, p in shapes]
    half_p, half_m = _forged(mat["cproofs"][7])
    for half in (half_p, half_m):   # neighbours, one half each at the same offset
        g = group(1, None)
        g[2][7] = half
        groups.append(g)
        want.append(False)
    for (blobs, cms, proofs), w in zip(groups, want):
        n = len(blobs)
        assert oracle.verify_cell_kzg_proof_batch([mat["cm"]] * (128 * n), list(range(128)) * n, list(mat["cells"]) * n, proofs) is w
    ok, st = hip.verify_blob_cell_kzg_proof_batch_groups(groups)
    assert st == [0] * len(groups) and ok == want


# ---- the two _locate calls ----

LOCATE_PAIRS = [(2, 0, 1), (70, 1, 64), (256, 5, 255), (258, 1, 257)]


@pytest.mark.parametrize("max_checks", [1024, 0])
@pytest.mark.parametrize("n,i,j", LOCATE_PAIRS)
def test_point_locate_finds_both_halves(hip, mat, n, i, j, max_checks):
    """expected: the oracle's single-item verdicts (asserted in `mat`): both forged halves false, every other item
    true.  Equal weights at (i, j) would pass the chunk's root check and report all n valid.  max_checks = 0 hands
    over to the per-lane check as soon as the root check fails."""
    proofs = _with_pair([mat["pproof"]] * n, i, j, mat["point_pair"])
    with _Option(hip, b"locate_max_checks", max_checks, 1024):
        ok, st, _ = hip.verify_kzg_proof_batch_locate([mat["cm"]] * n, [mat["z"]] * n, [mat["y"]] * n, proofs)
    assert st == [0] * n and ok == [k not in (i, j) for k in range(n)]


@pytest.mark.parametrize("max_checks", [1024, 0])
@pytest.mark.parametrize("n,i,j", LOCATE_PAIRS[:3])
def test_blob_locate_finds_both_halves(hip, oracle, mat, n, i, j, max_checks):
    blobs, cms, forged = _blob_batch(oracle, mat, n, i, j)
    with _Option(hip, b"locate_max_checks", max_checks, 1024):
        ok, st, _ = hip.verify_blob_kzg_proof_batch_locate(blobs, cms, forged)
    assert st == [0] * n and ok == [k not in (i, j) for k in range(n)]
