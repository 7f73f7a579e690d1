"""ckzg_hip_verify_blob_cell_kzg_proof_batch_groups: blobs against their 128 cell proofs each, many groups in one call,
one verdict per group.  Every group must come out as the reference functions composed on its slice do:
compute_cells of every blob, then verify_cell_kzg_proof_batch over all their cells with the blob's commitment repeated
128 times and the indices 0..127.  Expected values come from the consensus-spec vectors, from the CPU oracle, or from
how the data was made (openings the oracle computed are valid, however often they are repeated) -- never from the
library under test."""
import ctypes as C
import hashlib
import os
import re
import threading

import pytest

import g1_points as GP
from golden_util import case_names, get_case
from kzg_ctypes import HIP_SO, Kzg, KzgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BADARGS = 1
NAME = "ckzg_hip_verify_blob_cell_kzg_proof_batch_groups"
NOT_G1 = GP.by_label("Q+T11").data
OFF_CURVE = GP.by_label("off_curve").data
INFINITY = GP.by_label("inf").data


def _chunk_blobs():
    src = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    return int(re.search(r"#define CKZG_HIP_BLOB_CELL_GROUPS_CHUNK_BLOBS (\d+)", src).group(1))


def _check(got, expected, names=None):
    ok, st = got
    assert len(ok) == len(expected) and len(st) == len(expected)
    for g, exp in enumerate(expected):
        what = (g, names[g] if names else None, ok[g], st[g], exp)
        if exp is None:
            assert st[g] == BADARGS and ok[g] is False, what
        else:
            assert st[g] == 0 and ok[g] is exp, what


def _oracle_composition(oracle, group, known_cells=None):
    """what the reference functions give on one group: True / False, or None for a call that fails"""
    blobs, commitments, proofs = group
    cells = []
    for b in blobs:
        try:
            cells += (known_cells or {}).get(b) or oracle.compute_cells(b)
        except KzgError:
            return None
    try:
        return oracle.verify_cell_kzg_proof_batch([c for c in commitments for _ in range(128)], list(range(128)) * len(blobs),
                                                  cells, proofs)
    except KzgError:
        return None


# ---- the spec vectors ----

@pytest.mark.gpu
def test_spec_vectors_of_compute_cells_and_kzg_proofs_as_groups_of_one_call(hip, oracle):
    valid, invalid, left_out = [], [], 0
    for name in case_names("compute_cells_and_kzg_proofs"):
        inp, exp = get_case("compute_cells_and_kzg_proofs", name)
        blob = inp["blob"]
        if blob is None or len(blob) != 131072:
            left_out += 1
            continue
        if exp is None:
            invalid.append((name, blob))
        else:
            assert len(exp[1]) == 128
            valid.append(((([blob], [oracle.blob_to_kzg_commitment(blob)], list(exp[1]))), True, name))
    assert (len(valid), len(invalid), left_out) == (7, 2, 2)
    # a blob that compute_cells must reject, under valid points -> BADARGS
    bad = [(([blob], valid[i][0][1], valid[i][0][2]), None, name) for i, (name, blob) in enumerate(invalid)]
    # every invalid group between two that are not
    groups = [g for pair in zip(valid, bad) for g in pair] + valid[len(bad):]
    exp = [g[1] for g in groups]
    assert exp == [True, None, True, None, True, True, True, True, True]
    _check(hip.verify_blob_cell_kzg_proof_batch_groups([g[0] for g in groups]), exp, [g[2] for g in groups])
    _check(hip.verify_blob_cell_kzg_proof_batch_groups([g[0] for g in groups[::-1]]), exp[::-1])
    for g in groups:
        _check(hip.verify_blob_cell_kzg_proof_batch_groups([g[0]]), [g[1]], [g[2]])


# ---- material from the oracle ----

def _blob(seed, i):
    return b"".join(b"\x00" + hashlib.sha256(b"blobcellgroups%d/%d/%d" % (seed, i, j)).digest()[:31] for j in range(4096))


@pytest.fixture(scope="module")
def material(oracle):
    """4 random blobs with commitments, cells and cell proofs from the CPU oracle: [(blob, commitment, cells, proofs)]"""
    out = []
    for i in range(4):
        blob = _blob(97, i)
        cells, proofs = oracle.compute_cells_and_kzg_proofs(blob)
        out.append((blob, oracle.blob_to_kzg_commitment(blob), cells, proofs))
    return out


def _group(material, which):
    """the group of the blobs material[w] for w in which (repeats allowed), as lists that a test may change"""
    return [[material[w][0] for w in which], [material[w][1] for w in which], [p for w in which for p in material[w][3]]]


def _set_element(blob, j, value):
    return blob[:32 * j] + value.to_bytes(32, "big") + blob[32 * j + 32:]


def _flip_low_bit(blob, j):
    v = int.from_bytes(blob[32 * j:32 * j + 32], "big") ^ 1
    assert v < R   # still canonical
    return _set_element(blob, j, v)


def _swap_proofs_5_and_6(grp, blob_in_group):
    p = grp[2]
    a = 128 * blob_in_group
    assert p[a + 5] != p[a + 6]
    p[a + 5], p[a + 6] = p[a + 6], p[a + 5]


SIZES = ([0], [1, 2], [3, 0, 1], [], [2], [0, 1, 2, 3, 1, 0])   # groups of 1, 2, 3, 0, 1 and 6 blobs, the 6 with repeats


def _mixed_sizes(material):
    return [_group(material, which) for which in SIZES]


# one change per group: (blobs of the group, the change, expected)
def _changes():
    def swapped(g):
        _swap_proofs_5_and_6(g, len(g[0]) - 1)

    def proofs_of_another_blob(g):   # blob A's proofs under blob B
        assert g[0][0] != g[0][1]
        g[2][0:128] = g[2][128:256]

    def commitment_of_another_blob(g):
        assert g[1][0] != g[1][1]
        g[1][0] = g[1][1]

    def bit_in_element_0(g):
        g[0][0] = _flip_low_bit(g[0][0], 0)

    def bit_in_element_4095(g):
        g[0][-1] = _flip_low_bit(g[0][-1], 4095)

    def infinity_as_a_proof(g):
        g[2][128 + 77] = INFINITY

    def proof_outside_g1(g):   # the last proof of the group's last blob
        g[2][-1] = NOT_G1

    def commitment_outside_g1(g):
        g[1][1] = NOT_G1

    def proof_off_the_curve(g):
        g[2][3] = OFF_CURVE

    def modulus_in_the_second_blob(g):
        g[0][1] = _set_element(g[0][1], 4095, R)

    return [([2], swapped, False), ([0, 1], proofs_of_another_blob, False), ([3, 2, 1], commitment_of_another_blob, False),
            ([1], bit_in_element_0, False), ([0, 3], bit_in_element_4095, False), ([2, 0], infinity_as_a_proof, False),
            ([1, 3, 3], proof_outside_g1, None), ([0, 1, 2, 3, 1, 0], commitment_outside_g1, None),
            ([3], proof_off_the_curve, None), ([2, 1], modulus_in_the_second_blob, None)]


def _changed_call(material):
    """every changed group between unchanged ones of the mixed sizes; -> (groups, expected, indices of the changed)"""
    groups, exp, changed = [], [], []
    for i, (which, change, want) in enumerate(_changes()):
        groups.append(_group(material, SIZES[i % len(SIZES)]))
        exp.append(True)
        g = _group(material, which)
        change(g)
        changed.append(len(groups))
        groups.append(g)
        exp.append(want)
    groups.append(_group(material, SIZES[1]))
    exp.append(True)
    return groups, exp, changed


@pytest.mark.gpu
def test_mixed_sizes_in_one_call(hip, oracle, material):
    assert GP.classify(NOT_G1) == GP.NOT_IN_G1 and GP.classify(OFF_CURVE) == GP.BAD_ENCODING and GP.classify(INFINITY) == GP.VALID
    groups = _mixed_sizes(material)
    assert [len(g[0]) for g in groups] == [1, 2, 3, 0, 1, 6] and all(len(g[2]) == 128 * len(g[0]) for g in groups)
    assert len(set(groups[5][0])) < 6
    _check(hip.verify_blob_cell_kzg_proof_batch_groups(groups), [True] * 6)
    groups, exp, changed = _changed_call(material)
    assert (exp.count(True), exp.count(False), exp.count(None)) == (11, 6, 4)
    assert all(exp[i - 1] is True and exp[i + 1] is True for i in changed)
    _check(hip.verify_blob_cell_kzg_proof_batch_groups(groups), exp)
    # each kind of expected false or BADARGS, once with the oracle composition
    known = {m[0]: m[2] for m in material}
    for i in changed:
        assert _oracle_composition(oracle, groups[i], known) is exp[i], i
    # ... and every changed group alone: the path of a one-group call
    for i in changed:
        _check(hip.verify_blob_cell_kzg_proof_batch_groups([groups[i]]), [exp[i]])


@pytest.mark.gpu
def test_duplicate_commitment_in_a_group(hip, material):
    g = _group(material, [1, 1])
    other = _group(material, [0])
    _check(hip.verify_blob_cell_kzg_proof_batch_groups([other, g, other]), [True, True, True])
    _check(hip.verify_blob_cell_kzg_proof_batch_groups([g]), [True])
    g[2][128 + 9] = g[2][128 + 10]   # one copy's proof of cell 9
    _check(hip.verify_blob_cell_kzg_proof_batch_groups([other, g, other]), [True, False, True])
    _check(hip.verify_blob_cell_kzg_proof_batch_groups([g]), [False])


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [0, 1, 2, 3])
def test_a_non_canonical_blob_marks_its_own_group_only(hip, oracle, material, bad):
    """groups of 1, 2 and 1 blobs in one chunk; blob `bad` of the chunk -- the first one, either one of the middle group,
    the last one -- holds the modulus as a field element.  The flag is one word per blob, the half that folds the flags
    takes one per 2^bad_shift cells: only the group of that blob is C_KZG_BADARGS, the two others verify."""
    groups = [_group(material, w) for w in ([0], [1, 2], [3])]
    g, i = [(0, 0), (1, 0), (1, 1), (2, 0)][bad]
    groups[g][0][i] = _set_element(groups[g][0][i], 17, R)
    exp = [True] * 3
    exp[g] = None
    assert _oracle_composition(oracle, groups[g], {m[0]: m[2] for m in material}) is None   # (compute_cells rejects the blob)
    _check(hip.verify_blob_cell_kzg_proof_batch_groups(groups), exp)


def _raw_call(api, groups, with_status=True, start=None, null_data=False):
    g = len(groups)
    flat = [b"".join(x for grp in groups for x in grp[k]) for k in range(3)]
    if start is None:
        start = [0]
        for grp in groups:
            start.append(start[-1] + len(grp[0]))
    ok = (C.c_bool * max(g, 1))(*([True] * max(g, 1)))
    st = (C.c_uint8 * max(g, 1))(*([7] * max(g, 1)))
    f = getattr(api.lib, NAME)
    f.restype = C.c_int
    ret = f(ok, st if with_status else None, None if null_data else flat[0], flat[1], flat[2], (C.c_uint64 * len(start))(*start),
            C.c_uint64(g), api.sp)
    return ret, [bool(v) for v in ok[:g]], [int(v) for v in st[:g]]


@pytest.mark.gpu
def test_edges_of_the_argument_list(hip, material):
    f = getattr(hip.lib, NAME)
    f.restype = C.c_int
    assert f(None, None, None, None, None, None, C.c_uint64(0), hip.sp) == 0
    assert hip.verify_blob_cell_kzg_proof_batch_groups([]) == ([], [])
    empty = [[], [], []]
    assert hip.verify_blob_cell_kzg_proof_batch_groups([empty] * 5) == ([True] * 5, [0] * 5)
    groups = [_group(material, w) for w in ([0], [1, 2], [3], [2, 2], [1], [0, 3])]
    _swap_proofs_5_and_6(groups[2], 0)
    groups[4][2][127] = NOT_G1
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
    for start in ([1, 1, 3, 4, 6, 7, 9], [0, 1, 3, 2, 6, 7, 9]):
        assert _raw_call(hip, groups, start=start) == (BADARGS, [True] * 6, [7] * 6)
    # NULL data with a non-zero total
    assert _raw_call(hip, groups, null_data=True) == (BADARGS, [True] * 6, [7] * 6)


@pytest.mark.gpu
def test_chunk_boundary_inside_the_call_and_a_group_larger_than_a_chunk(hip, material):
    CH = _chunk_blobs()
    assert CH >= 8

    def call(sizes, bad_blobs):
        """groups of these sizes over the material repeated; the blobs (numbered through the call) in bad_blobs get two
        proofs swapped; -> what the call gives, what it must give"""
        groups, exp, at = [], [], 0
        for n in sizes:
            g = _group(material, [(at + i) % 4 for i in range(n)])
            hit = [b - at for b in bad_blobs if at <= b < at + n]
            for b in hit:
                _swap_proofs_5_and_6(g, b)
            groups.append(g)
            exp.append(not hit)
            at += n
        return hip.verify_blob_cell_kzg_proof_batch_groups(groups), exp

    # the call is cut behind the first group: CH - 1 + 2 blobs are more than a chunk
    got, exp = call([CH - 1, 2, 1], [])
    _check(got, exp)
    got, exp = call([CH - 1, 2, 1], [CH - 2, CH - 1])
    assert exp == [False, False, True]
    _check(got, exp)
    # a group of exactly a chunk, and one blob more: the larger-than-a-chunk route, cut after CH blobs
    for n in (CH, CH + 1):
        got, exp = call([n], [])
        _check(got, exp)
        for bad in ([CH - 1], [CH]) if n > CH else ([CH - 1],):
            got, exp = call([n], bad)
            assert exp == [False]
            _check(got, exp)
    # groups of one blob: the call is cut after CH groups
    got, exp = call([1] * (CH + 2), [CH - 1, CH])
    assert exp == [True] * (CH - 1) + [False, False, True]
    _check(got, exp)


@pytest.mark.gpu
def test_group_split_over_two_replicas(material):
    # (two table replicas on one GPU stand in for two devices: the same fan-out, and no second GPU is needed)
    groups, exp, _ = _changed_call(material)
    groups, exp = groups * 2, exp * 2   # (enough groups for both replicas to get a run)
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        _check(api.verify_blob_cell_kzg_proof_batch_groups(_mixed_sizes(material)), [True] * 6)
        _check(api.verify_blob_cell_kzg_proof_batch_groups(groups), exp)
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


@pytest.mark.gpu
def test_concurrent_callers(hip, material):
    sets = []
    for t in range(4):
        groups = [_group(material, SIZES[(t + i) % len(SIZES)]) for i in range(6 + t)]
        bad = next(i for i in range(t + 1, len(groups)) if groups[i][0])   # another group in every thread
        _swap_proofs_5_and_6(groups[bad], 0)
        sets.append((groups, [i != bad for i in range(len(groups))]))
    assert len({tuple(e) for _, e in sets}) == 4
    results, errors = [None] * 4, []

    def work(t):
        try:
            results[t] = hip.verify_blob_cell_kzg_proof_batch_groups(sets[t][0])
        except Exception as e:   # reported below
            errors.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors
    for t in range(4):
        _check(results[t], sets[t][1])


@pytest.mark.gpu
def test_binding_rejects_wrong_lengths(hip, material):
    g = _group(material, [0])
    for groups in ([[g[0], g[1], g[2][:127] + [g[2][127][:47]]]],   # a 47-byte proof
                   [[g[0], g[1], g[2][:127]]],                      # 127 proofs for one blob
                   [(g[0], g[1])]):                                 # a 2-tuple group
        with pytest.raises(KzgError):
            hip.verify_blob_cell_kzg_proof_batch_groups(groups)
