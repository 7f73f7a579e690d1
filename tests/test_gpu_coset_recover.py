"""GPU parity for ckzg_hip_recover_cosets_and_kzg_proofs_rows at every coset size 2^e, e = 0 .. 6: rows that hold
different cosets, recovered in one call, one status per row.  The reference is never the call under test: the extended
evaluations are the oracle's compute_cells_and_kzg_proofs, the proofs are ckzg_hip_compute_coset_kzg_proofs_batch of
the blob (which has its own tests), and at e = 6 also the oracle's recover_cells_and_kzg_proofs and the cell call by rows.
Everything is compared byte for byte."""
import ctypes as C
import os
import random
import re

import pytest

from conftest import ROOT
from test_gpu_commitment import rand_blob

pytestmark = pytest.mark.gpu
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
EVALS = 8192 * 32
ES = list(range(7))
NAME = "ckzg_hip_recover_cosets_and_kzg_proofs_rows"
CHUNK_ROWS = int(re.search(r"#define CKZG_HIP_COSET_RECOVER_CHUNK_ROWS (\d+)",
                           open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()).group(1))


@pytest.fixture(scope="module")
def full(oracle):
    """two random blobs, their extended evaluations (the oracle's 128 cells back to back) and the oracle's cell proofs"""
    out = []
    for i in range(2):
        blob = rand_blob(83, i)
        cells, proofs = oracle.compute_cells_and_kzg_proofs(blob)
        ext = b"".join(cells)
        assert len(ext) == EVALS and ext[:len(blob)] == blob
        out.append(dict(blob=blob, ext=ext, cells=cells, cell_proofs=proofs))
    return out


@pytest.fixture(scope="module")
def ref_proofs(hip, full):
    """e -> per blob the m proofs of ckzg_hip_compute_coset_kzg_proofs_batch, back to back"""
    cache = {}

    def get(e):
        if e not in cache:
            proofs, status = hip.compute_coset_kzg_proofs_batch([f["blob"] for f in full], e)
            assert status == [0, 0]
            cache[e] = [b"".join(p) for p in proofs]
        return cache[e]
    return get


def held_sets(e):
    """name -> held cosets"""
    m = 8192 >> e
    rnd = random.Random(40 + e)
    miss = lambda js: [c for c in range(m) if c not in set(js)]
    return {"all": list(range(m)),
            "one_missing": miss([rnd.randrange(m)]),
            "first_half_missing": list(range(m // 2, m)),
            "second_half_missing": list(range(m // 2)),
            "even_missing": list(range(1, m, 2)),
            "random_half": sorted(rnd.sample(range(m), m // 2)),
            "half_less_one_missing": miss(rnd.sample(range(m), m // 2 - 1)),
            "odd_count_missing": miss(rnd.sample(range(m), m // 2 - 5))}     # no multiple of any parts > 1


def cut(ext, idx, e):
    item = 32 << e
    return b"".join(ext[c * item:(c + 1) * item] for c in idx)


def raw_call(api, rows, e, want_evals=True, want_proofs=True, status=True, start=None, sentinel=0xa5):
    """the C call over buffers filled with a sentinel byte; rows: (indices, bytes).  Returns (ret, evals, proofs, status)"""
    nr, ps = len(rows), 48 * (8192 >> min(e, 6))
    if start is None:
        start = [0]
        for idx, _ in rows:
            start.append(start[-1] + len(idx))
    flat = [i for idx, _ in rows for i in idx]
    f = getattr(api.lib, NAME)
    f.restype = C.c_int
    fill = lambda n: (C.c_char * n).from_buffer(bytearray([sentinel]) * n)
    rv = fill(max(nr, 1) * EVALS) if want_evals else None
    rp = fill(max(nr, 1) * ps) if want_proofs else None
    st = (C.c_uint8 * max(nr, 1))(*([sentinel] * max(nr, 1))) if status else None
    ret = f(rv, rp, st, (C.c_uint64 * max(len(flat), 1))(*flat), b"".join(b for _, b in rows), (C.c_uint64 * len(start))(*start),
            C.c_uint64(nr), C.c_uint32(e), api.sp)
    return ret, (rv.raw if want_evals else None), (rp.raw if want_proofs else None), (list(st)[:nr] if status else None)


@pytest.mark.parametrize("e", ES)
def test_rows_return_the_oracles_bytes_and_the_openings_proofs(hip, full, ref_proofs, e):
    sets = held_sets(e)
    m = 8192 >> e
    assert len(sets["random_half"]) == m // 2 and len(sets["half_less_one_missing"]) == m // 2 + 1
    names = list(sets) + ["random_half"]                      # the last row shares its set with an earlier one
    blobs = [r % 2 for r in range(len(names))]
    assert blobs[names.index("random_half")] != blobs[-1]     # ... and holds another blob
    rows = [(sets[n], cut(full[b]["ext"], sets[n], e)) for n, b in zip(names, blobs)]
    want_p = ref_proofs(e)
    if e >= 2:
        ev, pr, st = hip.recover_cosets_and_kzg_proofs_rows(rows, e)
        with_proofs = list(range(len(rows)))
    else:   # the expensive sizes: proofs for two rows only
        ev, _, st = hip.recover_cosets_and_kzg_proofs_rows(rows, e, True, False)
        with_proofs = [names.index("odd_count_missing"), len(rows) - 1]
        ev2, pr2, st2 = hip.recover_cosets_and_kzg_proofs_rows([rows[r] for r in with_proofs], e)
        assert st2 == [0, 0]
        assert ev2 == [ev[r] for r in with_proofs]
        pr = {r: pr2[i] for i, r in enumerate(with_proofs)}
    assert st == [0] * len(rows)
    for r, b in enumerate(blobs):
        assert ev[r] == full[b]["ext"], "evaluations of row %d (%s)" % (r, names[r])
    for r in with_proofs:
        assert pr[r] == want_p[blobs[r]], "proofs of row %d (%s)" % (r, names[r])


@pytest.mark.parametrize("e", [1, 4])
def test_either_output_may_be_null(hip, full, ref_proofs, e):
    sets = held_sets(e)
    rows = [(sets[n], cut(full[b]["ext"], sets[n], e)) for n, b in (("random_half", 0), ("all", 1))]
    ret, ev, none_p, st = raw_call(hip, rows, e, True, False)
    assert ret == 0 and none_p is None and st == [0, 0]
    assert ev == full[0]["ext"] + full[1]["ext"]
    ret, none_e, pr, st = raw_call(hip, rows, e, False, True, status=False)
    assert ret == 0 and none_e is None and st is None
    assert pr == ref_proofs(e)[0] + ref_proofs(e)[1]
    ret, ev, pr, st = raw_call(hip, rows, e, False, False)
    assert ret == 1 and st == [0xa5, 0xa5]


def _mixed_with_invalid(full, e):
    m = 8192 >> e
    sets = held_sets(e)
    ext = [f["ext"] for f in full]
    junk = lambda idx: (idx, bytes((32 << e) * len(idx)))
    rows = [(sets["random_half"], cut(ext[0], sets["random_half"], e)),
            junk(list(range(m // 2 - 1))),                              # too few
            (sets["all"], cut(ext[1], sets["all"], e)),
            junk(list(range(m // 2 - 1)) + [m]),                        # an index = m
            junk(list(range(m // 2 - 1)) + [m // 2 - 2]),               # a repeated index
            (sets["even_missing"], cut(ext[1], sets["even_missing"], e)),
            junk([]),                                                   # an empty slice
            junk(list(range(m)) + [m]),                                 # too many
            (sets["random_half"], cut(ext[1], sets["random_half"], e))]
    return rows, [0, None, 1, None, None, 1, None, None, 1]


@pytest.mark.parametrize("e", [0, 3])
def test_invalid_rows_keep_the_sentinel_and_their_neighbours_are_recovered(hip, full, ref_proofs, e):
    rows, blobs = _mixed_with_invalid(full, e)
    ps = 48 * (8192 >> e)
    ret, ev, pr, st = raw_call(hip, rows, e, True, e == 3)
    assert ret == 1
    assert st == [0 if b is not None else 1 for b in blobs]
    for r, b in enumerate(blobs):
        got = ev[r * EVALS:(r + 1) * EVALS]
        assert got == (full[b]["ext"] if b is not None else b"\xa5" * EVALS), "row %d" % r
        if pr is not None:
            assert pr[r * ps:(r + 1) * ps] == (ref_proofs(e)[b] if b is not None else b"\xa5" * ps), "proofs of row %d" % r


def test_at_e6_the_call_is_the_cell_call_by_rows_and_the_oracle(hip, oracle, full):
    """The two entries run one code path at e = 6 (they differ in the rows of a chunk), so their equality is an identity
    check of the entries' argument handling; what pins the bytes is the oracle."""
    e = 6
    rows, blobs = _mixed_with_invalid(full, e)
    ret, ev, pr, st = raw_call(hip, rows, e)
    nr = len(rows)
    idx = [i for ix, _ in rows for i in ix]
    start = [0]
    for ix, _ in rows:
        start.append(start[-1] + len(ix))
    f = hip.lib.ckzg_hip_recover_cells_and_kzg_proofs_rows
    f.restype = C.c_int
    fill = lambda n: (C.c_char * n).from_buffer(bytearray([0xa5]) * n)
    rc2, rp2, st2 = fill(nr * EVALS), fill(nr * 128 * 48), (C.c_uint8 * nr)(*([0xa5] * nr))
    ret2 = f(rc2, rp2, st2, (C.c_uint64 * len(idx))(*idx), b"".join(b for _, b in rows), (C.c_uint64 * (nr + 1))(*start),
             C.c_uint64(nr), hip.sp)
    assert (ret, st) == (ret2, list(st2)) and ret == 1
    assert ev == rc2.raw and pr == rp2.raw
    for r in (0, 5):
        ix, data = rows[r]
        ec, ep = oracle.recover_cells_and_kzg_proofs(ix, [data[2048 * i:2048 * (i + 1)] for i in range(len(ix))])
        assert ev[r * EVALS:(r + 1) * EVALS] == b"".join(ec) == full[blobs[r]]["ext"]
        assert pr[r * 128 * 48:(r + 1) * 128 * 48] == b"".join(ep) == b"".join(full[blobs[r]]["cell_proofs"])


@pytest.mark.parametrize("e", [0, 5])
def test_a_non_canonical_value_flags_its_row_only(hip, full, e):
    sets = held_sets(e)
    idx = sets["random_half"]
    good = cut(full[0]["ext"], idx, e)
    at = 32 * ((len(idx) << e) - 3)
    bad = good[:at] + R.to_bytes(32, "big") + good[at + 32:]
    rows = [(idx, good), (idx, bad), (sets["one_missing"], cut(full[1]["ext"], sets["one_missing"], e))]
    ret, ev, _, st = raw_call(hip, rows, e, True, False)
    assert ret == 1 and st == [0, 1, 0]
    assert ev[:EVALS] == full[0]["ext"] and ev[2 * EVALS:] == full[1]["ext"]


def test_a_coset_size_the_library_does_not_have(hip, full):
    rows = [(list(range(64)), full[0]["ext"][:64 * 2048])]
    ret, ev, pr, st = raw_call(hip, rows, 7)
    assert ret == 1
    assert ev == b"\xa5" * EVALS and pr == b"\xa5" * len(pr) and st == [0xa5]


def test_malformed_row_start_and_empty_call(hip, full):
    e = 4
    idx = held_sets(e)["random_half"]
    rows = [(idx, cut(full[0]["ext"], idx, e))] * 2
    n = len(idx)
    for start in ([1, n, 2 * n], [0, 2 * n, n]):
        ret, ev, pr, st = raw_call(hip, rows, e, start=start)
        assert ret == 1 and ev == b"\xa5" * len(ev) and pr == b"\xa5" * len(pr) and st == [0xa5, 0xa5]
    f = getattr(hip.lib, NAME)
    f.restype = C.c_int
    assert f(None, None, None, None, None, None, C.c_uint64(0), C.c_uint32(e), hip.sp) == 0
    start = (C.c_uint64 * 2)(0, n)
    out = C.create_string_buffer(EVALS)
    assert f(out, None, None, None, None, start, C.c_uint64(1), C.c_uint32(e), hip.sp) == 1     # NULL inputs with work to do
    assert out.raw == bytes(EVALS)


def test_more_rows_than_one_chunk_with_an_invalid_row_on_the_boundary(hip, full):
    """CHUNK_ROWS + 1 valid rows at e = 5, evaluations only, and an invalid caller row between the last row of the first
    chunk and the first row of the second"""
    e = 5
    sets = held_sets(e)
    names = ["random_half", "even_missing", "odd_count_missing", "all"]
    pieces = {(b, n): cut(full[b]["ext"], sets[n], e) for b in range(2) for n in names}
    pick = [((r + r // 3) % 2, names[(r + r // 7) % 4]) for r in range(CHUNK_ROWS + 1)]
    rows = [(sets[n], pieces[(b, n)]) for b, n in pick]
    rows.insert(CHUNK_ROWS, (list(range(5)), bytes(5 * (32 << e))))
    blobs = [b for b, _ in pick]
    blobs.insert(CHUNK_ROWS, None)
    ret, ev, _, st = raw_call(hip, rows, e, True, False)
    assert ret == 1 and st == [0 if b is not None else 1 for b in blobs]
    for r, b in enumerate(blobs):   # every row, both sides of the boundary among them
        want = full[b]["ext"] if b is not None else b"\xa5" * EVALS
        assert ev[r * EVALS:(r + 1) * EVALS] == want, "row %d" % r


def test_proofs_across_the_openings_sub_batch(hip, full, ref_proofs):
    """18 rows with proofs at e = 4: the proof tail runs the openings in sub-batches of 16 rows"""
    e = 4
    sets = held_sets(e)
    names = ["random_half", "first_half_missing", "all"]
    pick = [((r + r // 5) % 2, names[r % 3]) for r in range(18)]
    rows = [(sets[n], cut(full[b]["ext"], sets[n], e)) for b, n in pick]
    ev, pr, st = hip.recover_cosets_and_kzg_proofs_rows(rows, e)
    assert st == [0] * 18
    for r, (b, _) in enumerate(pick):
        assert ev[r] == full[b]["ext"], "row %d" % r
        assert pr[r] == ref_proofs(e)[b], "proofs of row %d" % r


def test_recovered_cosets_verify(hip, full):
    """round trip at e = 2: recovered values and proofs of sampled cosets pass ckzg_hip_verify_coset_kzg_proof_batch"""
    e, m, item = 2, 2048, 128
    sets = held_sets(e)
    rows = [(sets["random_half"], cut(full[0]["ext"], sets["random_half"], e)),
            (sets["odd_count_missing"], cut(full[1]["ext"], sets["odd_count_missing"], e))]
    ev, pr, st = hip.recover_cosets_and_kzg_proofs_rows(rows, e)
    assert st == [0, 0]
    commitments = [hip.blob_to_kzg_commitment(f["blob"]) for f in full]
    rnd = random.Random(5)
    items = [(r, c) for r in range(2) for c in [0, m - 1] + rnd.sample(range(m), 14)]
    args = ([commitments[r] for r, _ in items], [c for _, c in items], [ev[r][c * item:(c + 1) * item] for r, c in items],
            [pr[r][48 * c:48 * c + 48] for r, c in items])
    assert hip.verify_coset_kzg_proof_batch(*args, e) is True
    wrong = list(args[2])
    wrong[3] = wrong[4]
    assert hip.verify_coset_kzg_proof_batch(args[0], args[1], wrong, args[3], e) is False


# ---- e = 6 through the coset entry: the cell call's code, FK20 proof tail included ----

E6_ROWS = [(0, "random_half"), (1, "first_half_missing"), None, (0, "held_70"), (1, "all")]


@pytest.fixture(scope="module")
def e6(oracle, full):
    """(blob, set name) -> (indices, held bytes, the oracle's recovered row, the oracle's 128 proofs) for the valid rows of
    E6_ROWS: two distinct half-sets, a row of 70 cosets and a full row.  The oracle runs once per row."""
    sets = dict(held_sets(6), held_70=sorted(random.Random(46).sample(range(128), 70)))
    assert len(sets["random_half"]) == len(sets["first_half_missing"]) == 64 and sets["random_half"] != sets["first_half_missing"]
    out = {}
    for key in E6_ROWS:
        if key is None:
            continue
        b, name = key
        idx = sets[name]
        data = cut(full[b]["ext"], idx, 6)
        ec, ep = oracle.recover_cells_and_kzg_proofs(idx, [data[2048 * i:2048 * (i + 1)] for i in range(len(idx))])
        out[key] = (idx, data, b"".join(ec), b"".join(ep))
    return out


def _e6_rows(e6, keys):
    """rows for raw_call; None is the invalid row: 63 cosets"""
    return [(e6[k][0], e6[k][1]) if k is not None else (list(range(63)), bytes(63 * 2048)) for k in keys]


def test_e6_proofs_only_with_an_invalid_row_in_the_middle(hip, e6):
    """recovered_evals NULL: the FK20 tail on an image that is never made final"""
    ret, none_e, pr, st = raw_call(hip, _e6_rows(e6, E6_ROWS), 6, False, True)
    assert ret == 1 and none_e is None
    assert st == [0, 0, 1, 0, 0]
    for r, k in enumerate(E6_ROWS):
        want = e6[k][3] if k is not None else b"\xa5" * (128 * 48)
        assert pr[r * 128 * 48:(r + 1) * 128 * 48] == want, "proofs of row %d" % r


def test_e6_both_outputs_are_the_same_bytes_through_both_entries(hip, e6):
    """one code path behind both entries: their equality checks the entries, the oracle pins the bytes"""
    rows = _e6_rows(e6, E6_ROWS)
    ret, ev, pr, st = raw_call(hip, rows, 6)
    nr = len(rows)
    idx = [i for ix, _ in rows for i in ix]
    start = [0]
    for ix, _ in rows:
        start.append(start[-1] + len(ix))
    f = hip.lib.ckzg_hip_recover_cells_and_kzg_proofs_rows
    f.restype = C.c_int
    fill = lambda n: (C.c_char * n).from_buffer(bytearray([0xa5]) * n)
    rc2, rp2, st2 = fill(nr * EVALS), fill(nr * 128 * 48), (C.c_uint8 * nr)(*([0xa5] * nr))
    ret2 = f(rc2, rp2, st2, (C.c_uint64 * len(idx))(*idx), b"".join(b for _, b in rows), (C.c_uint64 * (nr + 1))(*start),
             C.c_uint64(nr), hip.sp)
    assert ret == ret2 == 1 and st == list(st2) == [0, 0, 1, 0, 0]
    assert ev == rc2.raw and pr == rp2.raw
    for r, k in enumerate(E6_ROWS):
        want_e, want_p = (e6[k][2], e6[k][3]) if k is not None else (b"\xa5" * EVALS, b"\xa5" * (128 * 48))
        assert ev[r * EVALS:(r + 1) * EVALS] == want_e, "evaluations of row %d" % r
        assert pr[r * 128 * 48:(r + 1) * 128 * 48] == want_p, "proofs of row %d" % r


def test_e6_nine_rows_piped_on_the_other_proof_path(hip_fk20, e6):
    """nine rows: the first size whose outputs go back through the pipe; with the low-latency proof path disabled, so
    that the coset entry reaches both FK20 proof paths as the cell entry does"""
    valid = [k for k in E6_ROWS if k is not None]
    keys = [valid[(r + r // 4) % 4] for r in range(9)]
    ret, ev, pr, st = raw_call(hip_fk20, _e6_rows(e6, keys), 6)
    assert ret == 0 and st == [0] * 9
    for r, k in enumerate(keys):
        assert ev[r * EVALS:(r + 1) * EVALS] == e6[k][2], "evaluations of row %d" % r
        assert pr[r * 128 * 48:(r + 1) * 128 * 48] == e6[k][3], "proofs of row %d" % r
