"""ckzg_hip_verify_blob_kzg_proof_batch_groups: verify_blob_kzg_proof_batch over many groups in one call, one verdict
per group.  Every group must come out exactly as the single call on its slice does.  Expected values come from the
consensus-spec vectors, from the CPU oracle, or from how the data was made (a blob proof the oracle computed is valid,
however often it is repeated) -- never from the library under test."""
import ctypes as C
import hashlib
import importlib.util
import os
import random
import re
import threading

import pytest

import g1_points as GP
from golden_util import case_names, get_case
from kzg_ctypes import HIP_SO, Kzg, KzgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BADARGS = 1
BLOB = 131072
NAME = "ckzg_hip_verify_blob_kzg_proof_batch_groups"
NOT_G1 = GP.by_label("Q+T11").data


def _limit(which):
    src = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    return int(re.search(r"#define CKZG_HIP_BLOB_GROUPS_CHUNK_%s (\d+)" % which, src).group(1))


def _well_formed(blobs, commitments, proofs):
    return (all(v is not None for v in (blobs, commitments, proofs)) and len({len(blobs), len(commitments), len(proofs)}) == 1 and
            all(v is not None and len(v) == BLOB for v in blobs) and all(v is not None and len(v) == 48 for v in commitments + proofs))


def _spec_groups():
    """(((blobs, commitments, proofs), expected, name) per well-formed vector, vectors left out) for the batch vectors and
    for the single-blob vectors as groups of one; expected is True / False, or None for a call that must fail"""
    batch, single, left = [], [], [0, 0]
    for name in case_names("verify_blob_kzg_proof_batch"):
        inp, exp = get_case("verify_blob_kzg_proof_batch", name)
        grp = (inp["blobs"], inp["commitments"], inp["proofs"])
        if not _well_formed(*grp):
            left[0] += 1
            continue
        batch.append((grp, exp, name))
    for name in case_names("verify_blob_kzg_proof"):
        inp, exp = get_case("verify_blob_kzg_proof", name)
        grp = ([inp["blob"]], [inp["commitment"]], [inp["proof"]])
        if not _well_formed(*grp):
            left[1] += 1
            continue
        single.append((grp, exp, name))
    return batch, single, left


def _check(got, expected, names=None):
    ok, st = got
    assert len(ok) == len(expected) and len(st) == len(expected)
    for g, exp in enumerate(expected):
        what = (g, names[g] if names else None, ok[g], st[g], exp)
        if exp is None:
            assert st[g] == BADARGS and ok[g] is False, what
        else:
            assert st[g] == 0 and ok[g] is exp, what


@pytest.mark.gpu
def test_all_well_formed_spec_vectors_as_groups_of_one_call(hip):
    batch, single, left = _spec_groups()
    bexp, sexp = [g[1] for g in batch], [g[1] for g in single]
    assert len(batch) == 15 and left[0] == 9
    assert (bexp.count(True), bexp.count(False), bexp.count(None)) == (7, 2, 6)
    assert sorted(len(g[0][0]) for g in batch) == [0, 1, 1, 2, 3, 4, 5, 6] + [7] * 7
    assert sum(len(g[0][0]) for g in batch) == 71
    assert len(single) == 23 and left[1] == 6
    assert (sexp.count(True), sexp.count(False), sexp.count(None)) == (9, 8, 6)
    # every failing group between two that are not
    groups = batch + single
    rest, invalid = [g for g in groups if g[1] is not None], [g for g in groups if g[1] is None]
    groups = [g for pair in zip(rest, invalid) for g in pair] + rest[len(invalid):]
    exp = [g[1] for g in groups]
    assert len(groups) == 38 and exp.count(None) == 12
    assert all(exp[i - 1] is not None and exp[i + 1] is not None for i in range(1, len(exp) - 1) if exp[i] is None)
    assert exp[0] is not None and exp[-1] is not None
    _check(hip.verify_blob_kzg_proof_batch_groups([g[0] for g in groups]), exp, [g[2] for g in groups])
    # ... in the opposite order too, and every group alone (the single-batch path of a one-group call)
    _check(hip.verify_blob_kzg_proof_batch_groups([g[0] for g in groups[::-1]]), exp[::-1])
    for g in groups:
        _check(hip.verify_blob_kzg_proof_batch_groups([g[0]]), [g[1]], [g[2]])


def _blob(seed, i):
    return b"".join(b"\x00" + hashlib.sha256(b"blobgroups%d/%d/%d" % (seed, i, j)).digest()[:31] for j in range(4096))


@pytest.fixture(scope="module")
def material(oracle):
    """8 random blobs with their commitments and blob proofs from the CPU oracle"""
    blobs = [_blob(84, i) for i in range(8)]
    cm = [oracle.blob_to_kzg_commitment(b) for b in blobs]
    return blobs, cm, [oracle.compute_blob_kzg_proof(b, c) for b, c in zip(blobs, cm)]


def _group(material, n, first=0):
    """n valid blobs: the base blobs in turn, starting with blob `first`"""
    return [[v[(first + i) % 8] for i in range(n)] for v in material]


def _flip_lowest_bit(blob, element):
    b = bytearray(blob)
    b[32 * element + 31] ^= 1
    assert int.from_bytes(b[32 * element:32 * element + 32], "big") < R   # still canonical
    return bytes(b)


def _with_r(blob, element):
    return blob[:32 * element] + R.to_bytes(32, "big") + blob[32 * element + 32:]


# The single path's SMALL_VERIFY_N = 3 and its call-table threshold of 8 as neighbours in one grouped call, both sides of
# a wave and a group that spans three waves for k_blob_group_ysum; every spoilt group between two untouched ones.
MIXED_SIZES = [1, 65, 0, 130, 2, 3, 64, 9, 4, 63, 8, 7, 2]


def _mixed_sizes(material, spoil):
    groups = [_group(material, n, first=g) for g, n in enumerate(MIXED_SIZES)]
    exp = [True] * len(groups)
    if spoil:
        assert sorted(set(MIXED_SIZES)) == [0, 1, 2, 3, 4, 7, 8, 9, 63, 64, 65, 130]
        g = groups[1]    # 65 blobs, the last one: the lowest bit of one field element
        g[0][64] = _flip_lowest_bit(g[0][64], 1234)
        exp[1] = False
        g = groups[3]    # 130 blobs: the last blob's proof and its neighbour's swapped
        assert g[2][129] != g[2][128]
        g[2][129], g[2][128] = g[2][128], g[2][129]
        exp[3] = False
        g = groups[5]    # another blob's commitment
        assert g[1][1] != g[1][2]
        g[1][1] = g[1][2]
        exp[5] = False
        groups[7][2][8] = NOT_G1    # a proof that is not in G1
        exp[7] = None
        groups[9][1][31] = NOT_G1   # a commitment that is the same point
        exp[9] = None
        groups[11][0][6] = _with_r(groups[11][0][6], 4095)   # a field element equal to r
        exp[11] = None
        assert all(exp[i - 1] is True and exp[i + 1] is True for i in range(len(exp)) if exp[i] is not True)
    return groups, exp


@pytest.mark.gpu
def test_mixed_group_sizes(hip, material):
    assert GP.classify(NOT_G1) == GP.NOT_IN_G1
    groups, exp = _mixed_sizes(material, False)
    _check(hip.verify_blob_kzg_proof_batch_groups(groups), exp)
    groups, exp = _mixed_sizes(material, True)
    assert (exp.count(True), exp.count(False), exp.count(None)) == (7, 3, 3)
    _check(hip.verify_blob_kzg_proof_batch_groups(groups), exp)


@pytest.mark.gpu
def test_challenges_hashed_on_the_gpu(hip, material):
    groups, exp = _mixed_sizes(material, True)
    assert hip.lib.ckzg_hip_set_option(b"gpu_sha_min", 1) == 0
    try:
        _check(hip.verify_blob_kzg_proof_batch_groups(groups), exp)
    finally:
        hip.lib.ckzg_hip_set_option(b"gpu_sha_min", 0)


def _random_partition(material, rnd):
    """256 blobs cut into groups of mixed sizes with empties; a dozen blobs, proofs or commitments spoilt"""
    blobs, cm, proofs = material
    flat = []
    for _ in range(256):
        b = rnd.randrange(8)
        flat.append([blobs[b], cm[b], proofs[b]])
    for _ in range(12):
        i, kind = rnd.randrange(256), rnd.randrange(5)
        if kind == 0:
            flat[i][2] = proofs[rnd.randrange(8)]                              # (maybe) another blob's proof
        elif kind == 1:
            flat[i][1] = cm[rnd.randrange(8)]                                  # (maybe) another blob's commitment
        elif kind == 2:
            flat[i][0] = _flip_lowest_bit(flat[i][0], rnd.randrange(4096))     # another polynomial
        elif kind == 3:
            flat[i][0] = _with_r(flat[i][0], rnd.randrange(4096))              # a non-canonical field element
        else:
            flat[i][1 + rnd.randrange(2)] = NOT_G1                             # a point outside G1
    sizes = [40, 0, 0, 1, 1, 1]
    left = 256 - sum(sizes)
    while left:
        n = min(left, rnd.choice((0, 1, 2, 3, 4, 6, 9, 17)))
        sizes.append(n)
        left -= n
    rnd.shuffle(sizes)
    groups, at = [], 0
    for n in sizes:
        groups.append([[t[k] for t in flat[at:at + n]] for k in range(3)])
        at += n
    assert at == 256
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_group_equals_the_single_call_on_its_slice_and_the_oracle(hip, oracle, material, seed):
    groups = _random_partition(material, random.Random(seed))
    assert any(len(g[0]) == 0 for g in groups) and any(len(g[0]) == 1 for g in groups) and any(len(g[0]) == 40 for g in groups)
    ok, st = hip.verify_blob_kzg_proof_batch_groups(groups)
    kinds = set()
    for g, grp in enumerate(groups):
        want = []
        for api in (oracle, hip):
            try:
                want.append((api.verify_blob_kzg_proof_batch(*grp), 0))
            except KzgError:   # the call failed: C_KZG_BADARGS
                want.append((False, BADARGS))
        assert want[0] == want[1] == (ok[g], st[g]), (g, len(grp[0]), want, ok[g], st[g])
        kinds.add(want[0])
    assert kinds == {(True, 0), (False, 0), (False, BADARGS)}


def _raw_call(api, groups, with_status=True, start=None):
    g = len(groups)
    flat = [[x for grp in groups for x in grp[k]] for k in range(3)]
    if start is None:
        start = [0]
        for grp in groups:
            start.append(start[-1] + len(grp[0]))
    ok = (C.c_bool * max(g, 1))(*([True] * max(g, 1)))
    st = (C.c_uint8 * max(g, 1))(*([7] * max(g, 1)))
    f = getattr(api.lib, NAME)
    f.restype = C.c_int
    ret = f(ok, st if with_status else None, b"".join(flat[0]), b"".join(flat[1]), b"".join(flat[2]),
            (C.c_uint64 * len(start))(*start), C.c_uint64(g), api.sp)
    return ret, [bool(v) for v in ok[:g]], [int(v) for v in st[:g]]


@pytest.mark.gpu
def test_edges_of_the_argument_list(hip, material):
    f = getattr(hip.lib, NAME)
    f.restype = C.c_int
    assert f(None, None, None, None, None, None, C.c_uint64(0), hip.sp) == 0
    assert hip.verify_blob_kzg_proof_batch_groups([]) == ([], [])
    empty = [[], [], []]
    assert hip.verify_blob_kzg_proof_batch_groups([empty] * 5) == ([True] * 5, [0] * 5)
    groups = [_group(material, 2, first=g) for g in range(6)]
    groups[2][2][0] = groups[2][2][1]          # a wrong proof
    groups[4][1][1] = NOT_G1                   # an invalid commitment
    exp = [True, True, False, True, None, True]
    ret, ok, st = _raw_call(hip, groups)
    assert ret == BADARGS
    _check((ok, st), exp)
    # status may be NULL
    ret2, ok2, st2 = _raw_call(hip, groups, with_status=False)
    assert (ret2, ok2, st2) == (BADARGS, ok, [7] * 6)
    ret3, ok3, _ = _raw_call(hip, groups[:4], with_status=False)
    assert (ret3, ok3) == (0, [True, True, False, True])
    # a malformed group_start: C_KZG_BADARGS, and nothing is written
    for start in ([1, 2, 4, 6, 8, 10, 12], [0, 2, 4, 3, 8, 10, 12]):
        assert _raw_call(hip, groups, start=start) == (BADARGS, [True] * 6, [7] * 6)


@pytest.mark.gpu
def test_chunk_boundary_inside_the_call_and_a_group_larger_than_a_chunk(hip, material):
    chunk = _limit("BLOBS")
    assert _limit("GROUPS") >= chunk // 8 + 4   # (the cut below is the blob limit's)
    per = 8
    # groups of 8 blobs: the call is cut after chunk / 8 groups; a wrong group on either side of the cut
    n = chunk // per + 4
    groups = [_group(material, per, first=g) for g in range(n)]
    exp = [True] * n
    for g in (chunk // per - 1, chunk // per, n - 1):
        groups[g][2][5], groups[g][2][6] = groups[g][2][6], groups[g][2][5]
        exp[g] = False
    groups[1][1][7] = NOT_G1
    exp[1] = None
    _check(hip.verify_blob_kzg_proof_batch_groups(groups), exp)
    # one group larger than a chunk between two small ones, valid and then with two proofs swapped
    big = _group(material, chunk + 1)
    small = [_group(material, 3), _group(material, 3, first=4)]
    small[1][2][0] = small[1][2][1]
    _check(hip.verify_blob_kzg_proof_batch_groups([small[0], big, small[1]]), [True, True, False])
    assert big[2][chunk - 1] != big[2][chunk]
    big[2][chunk - 1], big[2][chunk] = big[2][chunk], big[2][chunk - 1]
    _check(hip.verify_blob_kzg_proof_batch_groups([small[0], big, small[1]]), [True, False, False])


@pytest.mark.gpu
def test_600_groups_of_one_blob(hip, material):
    # 600 x (32 + 32) terms: past the quad limit, jobs padded to 32 terms
    blobs, cm, proofs = material
    rnd = random.Random(11)
    groups, exp = [], []
    for g in range(600):
        b, kind = rnd.randrange(8), g % 8
        p = proofs[b]
        if kind == 3:
            p = proofs[(b + 1) % 8]   # another blob's proof
        elif kind == 6:
            p = NOT_G1
        groups.append([[blobs[b]], [cm[b]], [p]])
        exp.append(False if kind == 3 else None if kind == 6 else True)
    assert (exp.count(False), exp.count(None)) == (75, 75)
    _check(hip.verify_blob_kzg_proof_batch_groups(groups), exp)


def _mixed(material, seed, n):
    rnd = random.Random(seed)
    groups, exp = [], []
    for _ in range(n):
        size = rnd.choice((1, 2, 3, 6, 9))
        g = _group(material, size, first=rnd.randrange(8))
        kind = rnd.randrange(4)
        if kind == 1:
            g[2][size - 1] = material[2][(material[2].index(g[2][size - 1]) + 1) % 8]   # another blob's proof
        elif kind == 2:
            g[1][rnd.randrange(size)] = NOT_G1
        groups.append(g)
        exp.append(False if kind == 1 else None if kind == 2 else True)
    return groups, exp


@pytest.mark.gpu
def test_group_split_over_two_replicas(material):
    # (two table replicas on one GPU stand in for two devices: the same fan-out, and no second GPU is needed)
    groups, exp = _mixed(material, 21, 100)
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        _check(api.verify_blob_kzg_proof_batch_groups(groups), exp)
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


@pytest.mark.gpu
def test_concurrent_callers(hip, material):
    sets = [_mixed(material, 100 + t, 6 + 5 * t) for t in range(8)]
    results, errors = [None] * 8, []

    def work(t):
        try:
            results[t] = hip.verify_blob_kzg_proof_batch_groups(sets[t][0])
        except Exception as e:   # reported below
            errors.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors
    for t in range(8):
        _check(results[t], sets[t][1])


NEW_KERNELS = ("k_blob_group_scalars", "k_blob_group_ysum")


def test_blob_group_kernels_use_no_scratch():
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
