"""ckzg_hip_verify_cell_kzg_proof_batch_groups: verify_cell_kzg_proof_batch over many groups in one call, one verdict
per group.  Every group must come out exactly as the single call on its slice does.  Expected values come from the
consensus-spec vectors, from the CPU oracle, or from how the data was made (openings the oracle computed are valid,
however often they are repeated) -- never from the library under test."""
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
NAME = "ckzg_hip_verify_cell_kzg_proof_batch_groups"


def _chunk_cells():
    src = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    return int(re.search(r"#define CKZG_HIP_CELL_GROUPS_CHUNK_CELLS (\d+)", src).group(1))


def _spec_groups():
    """((commitments, cell_indices, cells, proofs), expected) for every verify_cell_kzg_proof_batch vector whose inputs
    can be expressed as bytes; expected is True / False, or None for a call that must fail.  Second value: how many
    vectors were left out (missing or truncated inputs)."""
    groups, left_out = [], 0
    for name in case_names("verify_cell_kzg_proof_batch"):
        inp, exp = get_case("verify_cell_kzg_proof_batch", name)
        c, i, x, p = inp["commitments"], inp["cell_indices"], inp["cells"], inp["proofs"]
        if (any(v is None for v in (c, i, x, p)) or len({len(c), len(i), len(x), len(p)}) != 1 or
                any(v is None or len(v) != 48 for v in c + p) or any(v is None or len(v) != 2048 for v in x)):
            left_out += 1
            continue
        groups.append(((c, i, x, p), exp, name))
    return groups, left_out


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
    groups, left_out = _spec_groups()
    # every invalid group between two that are not
    rest, invalid = [g for g in groups if g[1] is not None], [g for g in groups if g[1] is None]
    groups = [g for pair in zip(rest, invalid) for g in pair] + rest[len(invalid):]
    exp = [g[1] for g in groups]
    assert len(groups) == 22 and left_out == 10
    assert (exp.count(True), exp.count(False), exp.count(None)) == (12, 3, 7)
    assert sum(len(g[0][2]) for g in groups) == 925
    assert {len(g[0][2]) for g in groups} == {0, 1, 2, 3, 4, 10, 128}
    assert all(exp[i - 1] is not None and exp[i + 1] is not None for i in range(1, len(exp) - 1) if exp[i] is None)
    assert exp[0] is not None and exp[-1] is not None
    _check(hip.verify_cell_kzg_proof_batch_groups([g[0] for g in groups]), exp, [g[2] for g in groups])
    # ... in the opposite order too, and every group alone (the single-batch path of a one-group call)
    _check(hip.verify_cell_kzg_proof_batch_groups([g[0] for g in groups[::-1]]), exp[::-1])
    for g in groups:
        _check(hip.verify_cell_kzg_proof_batch_groups([g[0]]), [g[1]], [g[2]])


def _blob(seed, i):
    return b"".join(b"\x00" + hashlib.sha256(b"cellgroups%d/%d/%d" % (seed, i, j)).digest()[:31] for j in range(4096))


@pytest.fixture(scope="module")
def material(oracle):
    """commitments, cells and proofs of 8 random blobs from the CPU oracle"""
    blobs = [_blob(83, i) for i in range(8)]
    cm = [oracle.blob_to_kzg_commitment(b) for b in blobs]
    cp = [oracle.compute_cells_and_kzg_proofs(b) for b in blobs]
    return cm, [c for c, _ in cp], [p for _, p in cp]


def _sidecars(material, rows):
    """the PeerDAS shape: group c = column c of every blob of a block of `rows` blobs (the 8 base blobs repeated)"""
    cm, cells, proofs = material
    return [[[cm[b % 8] for b in range(rows)], [c] * rows, [cells[b % 8][c] for b in range(rows)],
             [proofs[b % 8][c] for b in range(rows)]] for c in range(128)]


NOT_G1 = GP.by_label("Q+T11").data


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [8, 64])
def test_peerdas_shape(hip, material, rows):
    assert GP.classify(NOT_G1) == GP.NOT_IN_G1
    groups = _sidecars(material, rows)
    assert sum(len(g[2]) for g in groups) == 128 * rows
    _check(hip.verify_cell_kzg_proof_batch_groups(groups), [True] * 128)
    # four changes in one call
    exp = [True] * 128
    cell = bytearray(groups[5][2][3])
    cell[32 * 17 + 31] ^= 1          # the lowest bit of a field element: still canonical
    assert int.from_bytes(cell[32 * 17:32 * 18], "big") < R
    groups[5][2][3] = bytes(cell)
    exp[5] = False
    assert groups[77][3][1] != groups[77][3][2]   # (rows 1 and 2 are different blobs)
    groups[77][3][1], groups[77][3][2] = groups[77][3][2], groups[77][3][1]
    exp[77] = False
    groups[100][3][rows - 1] = NOT_G1
    exp[100] = None
    groups[101][0][0] = NOT_G1
    exp[101] = None
    _check(hip.verify_cell_kzg_proof_batch_groups(groups), exp)
    assert exp.count(True) == 124


@pytest.mark.gpu
def test_a_bad_commitment_that_all_groups_share(hip, material):
    groups = _sidecars(material, 8)
    for g in groups:
        g[0][2] = NOT_G1
    _check(hip.verify_cell_kzg_proof_batch_groups(groups), [None] * 128)


def _random_partition(material, rnd):
    """1,024 cells (with repeated commitments and repeated (column, blob) pairs) cut into groups of mixed sizes: empty
    groups, groups of one, one group of 600; some cells, proofs or commitments spoilt"""
    cm, cells, proofs = material
    flat = []
    for _ in range(1024):
        b, c = rnd.randrange(8), rnd.randrange(128) if rnd.random() < 0.8 else rnd.randrange(4)
        flat.append([cm[b], c, cells[b][c], proofs[b][c]])
    for _ in range(12):
        i, kind = rnd.randrange(1024), rnd.randrange(4)
        if kind == 0:
            flat[i][3] = proofs[rnd.randrange(8)][rnd.randrange(128)]   # another cell's proof
        elif kind == 1:
            flat[i][1] = (flat[i][1] + 1) % 128                         # the wrong column
        elif kind == 2:
            flat[i][0] = cm[rnd.randrange(8)]                           # (maybe) another blob's commitment
        else:
            flat[i][2] = flat[i][2][:64] + R.to_bytes(32, "big") + flat[i][2][96:]   # a non-canonical field element
    sizes = [600, 0, 0, 1, 1, 1]
    left = 1024 - sum(sizes)
    while left:
        n = min(left, rnd.choice((0, 1, 2, 3, 7, 31, 64, 65, 100)))
        sizes.append(n)
        left -= n
    rnd.shuffle(sizes)
    groups, at = [], 0
    for n in sizes:
        groups.append([[t[k] for t in flat[at:at + n]] for k in range(4)])
        at += n
    assert at == 1024
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_group_equals_the_single_call_on_its_slice_and_the_oracle(hip, oracle, material, seed):
    groups = _random_partition(material, random.Random(seed))
    assert any(len(g[2]) == 0 for g in groups) and any(len(g[2]) == 1 for g in groups) and any(len(g[2]) == 600 for g in groups)
    ok, st = hip.verify_cell_kzg_proof_batch_groups(groups)
    kinds = set()
    for g, grp in enumerate(groups):
        want = []
        for api in (oracle, hip):
            try:
                want.append((api.verify_cell_kzg_proof_batch(*grp), 0))
            except KzgError:   # the call failed: C_KZG_BADARGS
                want.append((False, BADARGS))
        assert want[0] == want[1] == (ok[g], st[g]), (g, len(grp[2]), want, ok[g], st[g])
        kinds.add(want[0])
    assert kinds == {(True, 0), (False, 0), (False, BADARGS)}


def _groups_with_rows(material, rows):
    """groups of 1, 2, 3, 1, ... cells, every cell of a group in a column of its own, so that the chunk has exactly `rows`
    distinct (group, column) pairs; an empty group last, so that one row is still a chunk of two groups"""
    cm, cells, proofs = material
    groups, at = [], 0
    while at < rows:
        n = min(len(groups) % 3 + 1, rows - at)
        ids = [((5 * i) % 8, (37 * i) % 128) for i in range(at, at + n)]
        groups.append([[cm[b] for b, _ in ids], [c for _, c in ids], [cells[b][c] for b, c in ids], [proofs[b][c] for b, c in ids]])
        at += n
    return groups + [[[], [], [], []]]


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 63, 64, 65])
def test_row_counts_around_a_workgroup_and_a_tile_of_rows(hip, oracle, material, rows):
    """The rows of a chunk lie back to back, unpadded: k_coset_group_interp takes 4 rows of 64 values a workgroup, and 64
    rows were the tile the rows were once padded to.  One forged cell in the last group that has cells."""
    groups = _groups_with_rows(material, rows)
    assert sum(len(set(g[1])) for g in groups) == rows and len(groups) >= 2 and all(len(g[2]) <= 3 for g in groups)
    forged = len(groups) - 2
    cell = bytearray(groups[forged][2][0])
    cell[32 * 17 + 31] ^= 1          # the lowest bit of a field element: still canonical
    assert int.from_bytes(cell[32 * 17:32 * 18], "big") < R
    groups[forged][2][0] = bytes(cell)
    ok, st = hip.verify_cell_kzg_proof_batch_groups(groups)
    for g, grp in enumerate(groups):
        want = [(api.verify_cell_kzg_proof_batch(*grp), 0) for api in (oracle, hip)]
        assert want[0] == want[1] == (ok[g], st[g]) == (g != forged, 0), (rows, g, want, ok[g], st[g])


def _raw_call(api, groups, with_status=True, start=None):
    g = len(groups)
    flat = [[x for grp in groups for x in grp[k]] for k in range(4)]
    if start is None:
        start = [0]
        for grp in groups:
            start.append(start[-1] + len(grp[2]))
    ok = (C.c_bool * max(g, 1))(*([True] * max(g, 1)))
    st = (C.c_uint8 * max(g, 1))(*([7] * max(g, 1)))
    f = getattr(api.lib, NAME)
    f.restype = C.c_int
    ret = f(ok, st if with_status else None, b"".join(flat[0]), (C.c_uint64 * max(len(flat[1]), 1))(*flat[1]), b"".join(flat[2]),
            b"".join(flat[3]), (C.c_uint64 * len(start))(*start), C.c_uint64(g), api.sp)
    return ret, [bool(v) for v in ok[:g]], [int(v) for v in st[:g]]


@pytest.mark.gpu
def test_edges_of_the_argument_list(hip, material):
    f = getattr(hip.lib, NAME)
    f.restype = C.c_int
    assert f(None, None, None, None, None, None, None, C.c_uint64(0), hip.sp) == 0
    assert hip.verify_cell_kzg_proof_batch_groups([]) == ([], [])
    empty = [[], [], [], []]
    assert hip.verify_cell_kzg_proof_batch_groups([empty] * 5) == ([True] * 5, [0] * 5)
    groups = _sidecars(material, 8)[:6]
    groups[2][3][0] = groups[2][3][1]   # a wrong proof
    groups[4][1][3] = 128               # an index out of range
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
    for start in ([1, 8, 16, 24, 32, 40, 48], [0, 8, 16, 15, 32, 40, 48]):
        assert _raw_call(hip, groups, start=start) == (BADARGS, [True] * 6, [7] * 6)


@pytest.mark.gpu
def test_chunk_boundary_inside_the_call_and_a_group_larger_than_a_chunk(hip, material):
    chunk = _chunk_cells()
    per = 512
    side = _sidecars(material, per)
    # groups of 512 cells: the call is cut after chunk / 512 groups; a wrong group on either side of the cut
    n = chunk // per + 8
    assert n * per > chunk > 4 * per
    groups = [[list(v) for v in side[g % 128]] for g in range(n)]
    exp = [True] * n
    for g in (chunk // per - 1, chunk // per, n - 1):
        groups[g][3][5], groups[g][3][6] = groups[g][3][6], groups[g][3][5]
        exp[g] = False
    groups[1][0][7] = NOT_G1
    exp[1] = None
    _check(hip.verify_cell_kzg_proof_batch_groups(groups), exp)
    # one group larger than a chunk between two small ones, valid and then with two proofs swapped
    rows = chunk // 128 + 1
    cm, cells, proofs = material
    big = [[cm[b % 8] for b in range(rows) for c in range(128)], [c for b in range(rows) for c in range(128)],
           [cells[b % 8][c] for b in range(rows) for c in range(128)], [proofs[b % 8][c] for b in range(rows) for c in range(128)]]
    assert len(big[2]) > chunk
    small = _sidecars(material, 8)
    small[1][3][0] = small[1][3][1]
    _check(hip.verify_cell_kzg_proof_batch_groups([small[0], big, small[1]]), [True, True, False])
    big[3][chunk], big[3][chunk + 1] = big[3][chunk + 1], big[3][chunk]
    _check(hip.verify_cell_kzg_proof_batch_groups([small[0], big, small[1]]), [True, False, False])


@pytest.mark.gpu
def test_4096_groups_of_one_cell(hip, material):
    cm, cells, proofs = material
    rnd = random.Random(11)
    groups, exp = [], []
    for g in range(4096):
        b, c = rnd.randrange(8), rnd.randrange(128)
        kind = rnd.randrange(8)
        p = proofs[b][c]
        if kind == 0:
            p = proofs[(b + 1) % 8][c]   # another blob's proof for this column
        elif kind == 1:
            p = NOT_G1
        groups.append([[cm[b]], [c], [cells[b][c]], [p]])
        exp.append(False if kind == 0 else None if kind == 1 else True)
    _check(hip.verify_cell_kzg_proof_batch_groups(groups), exp)


def _mixed(material, seed, n):
    rnd = random.Random(seed)
    side = _sidecars(material, 8)
    groups, exp = [], []
    for _ in range(n):
        g = [list(v) for v in side[rnd.randrange(128)]]
        kind = rnd.randrange(4)
        if kind == 1:
            g[3][2], g[3][3] = g[3][3], g[3][2]
        elif kind == 2:
            g[0][rnd.randrange(8)] = NOT_G1
        groups.append(g)
        exp.append(False if kind == 1 else None if kind == 2 else True)
    return groups, exp


@pytest.mark.gpu
def test_group_split_over_two_replicas(material):
    # (two table replicas on one GPU stand in for two devices: the same fan-out, and no second GPU is needed)
    groups, exp = _mixed(material, 21, 200)
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        _check(api.verify_cell_kzg_proof_batch_groups(groups), exp)
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


@pytest.mark.gpu
def test_concurrent_callers(hip, material):
    sets = [_mixed(material, 100 + t, 20 + 15 * t) for t in range(8)]
    results, errors = [None] * 8, []

    def work(t):
        try:
            results[t] = hip.verify_cell_kzg_proof_batch_groups(sets[t][0])
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


NEW_KERNELS = ("k_coset_group_rlc_scalars", "k_group_commit_weights", "k_coset_group_aggregate", "k_coset_group_interp",
               "k_coset_group_interp_sum", "k_group_gather_points")


def test_group_kernels_use_no_scratch():
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
