"""GPU parity for ckzg_hip_recover_cells_and_kzg_proofs_rows: rows that hold different cells, recovered in one call,
one status per row.  Every row must give exactly what recover_cells_and_kzg_proofs gives for that row alone
(src/eip7594/eip7594.c:177-304): the full row it was cut from, the library's own one-row call, the oracle; invalid
rows say so and leave their outputs alone without disturbing the others."""
import ctypes as C
import random

import pytest

from kzg_ctypes import HIP_SO, Kzg
from test_gpu_commitment import rand_blob

pytestmark = pytest.mark.gpu
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
CELLS, PROOFS = 128 * 2048, 128 * 48


def _sets():
    rnd = random.Random(2024)
    return {"even": list(range(0, 128, 2)), "first_64": list(range(64)), "last_64": list(range(64, 128)),
            "random_64": sorted(rnd.sample(range(128), 64)), "random_70": sorted(rnd.sample(range(128), 70)),
            "127_cells": sorted(rnd.sample(range(128), 127)), "all_128": list(range(128))}


# 13 rows over all seven sets, "random_70" and "first_64" twice and "even" three times, not sorted by set
ORDER = ["random_70", "even", "all_128", "first_64", "127_cells", "even", "last_64", "random_64", "first_64", "random_70",
         "all_128", "even", "127_cells"]


@pytest.fixture(scope="module")
def full(hip):
    """four random blobs with all their cells and proofs"""
    return [hip.compute_cells_and_kzg_proofs(rand_blob(71, i)) for i in range(4)]


def _mixed(full):
    sets = _sets()
    return [(sets[name], [full[r % len(full)][0][c] for c in sets[name]]) for r, name in enumerate(ORDER)]


def _expect_rows(full, rows_blob, got_cells, got_proofs):
    for r, b in enumerate(rows_blob):
        if got_cells is not None:
            assert got_cells[r] == full[b][0], "cells of row %d" % r
        if got_proofs is not None:
            assert got_proofs[r] == full[b][1], "proofs of row %d" % r


def test_mixed_sets_equal_full_rows_one_row_calls_and_oracle(hip, oracle, full):
    rows = _mixed(full)
    assert len(rows) >= 12 and len(set(ORDER)) == 7
    rc, rp, st = hip.recover_cells_and_kzg_proofs_rows(rows)
    assert st == [0] * len(rows)
    _expect_rows(full, [r % len(full) for r in range(len(rows))], rc, rp)
    for r, (idx, cells) in enumerate(rows):
        one_c, one_p = hip.recover_cells_and_kzg_proofs(idx, cells)
        assert rc[r] == one_c and rp[r] == one_p, "row %d against the one-row call" % r
    checked = set()
    for r in (0, 1, 3, 4):
        ec, ep = oracle.recover_cells_and_kzg_proofs(*rows[r])
        assert rc[r] == ec and rp[r] == ep, "row %d against the oracle" % r
        checked.add(ORDER[r])
    assert len(checked) >= 3


@pytest.mark.parametrize("which", ["direct", "fk20"])
def test_cells_only_and_proofs_only_on_both_proof_paths(hip, hip_fk20, full, which):
    api = hip_fk20 if which == "fk20" else hip
    rows = _mixed(full)
    blobs = [r % len(full) for r in range(len(rows))]
    rc, rp, st = api.recover_cells_and_kzg_proofs_rows(rows)
    c_only, none_p, st_c = api.recover_cells_and_kzg_proofs_rows(rows, True, False)
    none_c, p_only, st_p = api.recover_cells_and_kzg_proofs_rows(rows, False, True)
    assert none_p is None and none_c is None
    assert st == st_c == st_p == [0] * len(rows)
    _expect_rows(full, blobs, rc, rp)
    assert c_only == rc and p_only == rp


def _raw_call(api, rows, want_cells=True, want_proofs=True, status=True, start=None, sentinel=0xa5):
    """the C call over buffers filled with a sentinel byte; returns (ret, cells bytes, proofs bytes, status list)"""
    nr = len(rows)
    if start is None:
        start = [0]
        for idx, _ in rows:
            start.append(start[-1] + len(idx))
    flat_idx = [i for idx, _ in rows for i in idx]
    f = api.lib.ckzg_hip_recover_cells_and_kzg_proofs_rows
    f.restype = C.c_int
    rc = (C.c_char * (max(nr, 1) * CELLS)).from_buffer(bytearray([sentinel]) * (max(nr, 1) * CELLS)) if want_cells else None
    rp = (C.c_char * (max(nr, 1) * PROOFS)).from_buffer(bytearray([sentinel]) * (max(nr, 1) * PROOFS)) if want_proofs else None
    st = (C.c_uint8 * max(nr, 1))(*([sentinel] * max(nr, 1))) if status else None
    ret = f(rc, rp, st, (C.c_uint64 * max(len(flat_idx), 1))(*flat_idx), b"".join(c for _, cells in rows for c in cells),
            (C.c_uint64 * len(start))(*start), C.c_uint64(nr), api.sp)
    return ret, (rc.raw if want_cells else None), (rp.raw if want_proofs else None), (list(st)[:nr] if status else None)


def test_more_rows_than_one_chunk(hip, full):
    """1030 rows over five sets and four blobs: chunks of 512 + 512 + 6"""
    sets = _sets()
    names = ["random_70", "even", "last_64", "127_cells", "all_128"]
    cut = {(b, n): b"".join(full[b][0][c] for c in sets[n]) for b in range(4) for n in names}
    nr = 1030
    pick = [((7 * r + r // 5) % 4, names[(r + r // 9) % 5]) for r in range(nr)]
    idx = [i for _, n in pick for i in sets[n]]
    start = [0]
    for _, n in pick:
        start.append(start[-1] + len(sets[n]))
    f = hip.lib.ckzg_hip_recover_cells_and_kzg_proofs_rows
    f.restype = C.c_int
    rc, rp, st = C.create_string_buffer(nr * CELLS), C.create_string_buffer(nr * PROOFS), (C.c_uint8 * nr)()
    ret = f(rc, rp, st, (C.c_uint64 * len(idx))(*idx), b"".join(cut[p] for p in pick), (C.c_uint64 * (nr + 1))(*start),
            C.c_uint64(nr), hip.sp)
    assert ret == 0 and list(st) == [0] * nr
    craw, praw = rc.raw, rp.raw
    want_c = [b"".join(full[b][0]) for b in range(4)]
    want_p = [b"".join(full[b][1]) for b in range(4)]
    for r in range(nr):   # every row, both sides of both chunk boundaries among them
        b = pick[r][0]
        assert craw[r * CELLS:(r + 1) * CELLS] == want_c[b], "cells of row %d" % r
        assert praw[r * PROOFS:(r + 1) * PROOFS] == want_p[b], "proofs of row %d" % r
    assert len({pick[r] for r in (510, 511, 512, 513, 1023, 1024)}) > 3


def _bad_and_good(full):
    sets = _sets()

    def row(b, cols):
        return (list(cols), [full[b][0][c % 128] for c in cols])

    noncanon = row(2, sets["even"])
    cell = bytearray(noncanon[1][9])
    cell[64:96] = R.to_bytes(32, "big")
    noncanon[1][9] = bytes(cell)
    rows = [row(0, sets["random_70"]),
            row(1, range(63)),                                   # 63 cells
            row(1, sets["first_64"]),
            (list(range(128)) + [128], [full[0][0][c % 128] for c in range(129)]),   # 129 cells
            row(2, list(range(63)) + [128]),                     # an index of 128
            row(3, sets["all_128"]),
            row(0, list(range(62)) + [70, 69]),                  # a descending pair
            row(3, list(range(63)) + [62]),                      # a duplicated index
            row(2, sets["127_cells"]),
            noncanon,                                            # a field element >= r
            row(1, sets["even"])]
    structural = [1, 3, 4, 6, 7]
    blobs = {0: 0, 2: 1, 5: 3, 8: 2, 10: 1}
    return rows, structural, 9, blobs


def test_invalid_rows_between_good_rows(hip, full):
    rows, structural, noncanon, blobs = _bad_and_good(full)
    ret, craw, praw, st = _raw_call(hip, rows)
    assert ret == 1
    assert st == [int(r in structural or r == noncanon) for r in range(len(rows))]
    for r in structural:   # not written: still the sentinel
        assert craw[r * CELLS:(r + 1) * CELLS] == b"\xa5" * CELLS
        assert praw[r * PROOFS:(r + 1) * PROOFS] == b"\xa5" * PROOFS
    for r, b in blobs.items():
        assert craw[r * CELLS:(r + 1) * CELLS] == b"".join(full[b][0]), "cells of row %d" % r
        assert praw[r * PROOFS:(r + 1) * PROOFS] == b"".join(full[b][1]), "proofs of row %d" % r
    # the same without a status array, and through the binding
    ret2, craw2, praw2, _ = _raw_call(hip, rows, status=False)
    assert ret2 == 1
    for r in list(blobs) + structural:
        assert craw2[r * CELLS:(r + 1) * CELLS] == craw[r * CELLS:(r + 1) * CELLS]
        assert praw2[r * PROOFS:(r + 1) * PROOFS] == praw[r * PROOFS:(r + 1) * PROOFS]
    rc, rp, st3 = hip.recover_cells_and_kzg_proofs_rows(rows)
    assert st3 == st
    for r in range(len(rows)):
        assert (rc[r] is None) == (st[r] != 0) and (rp[r] is None) == (st[r] != 0)
        if r in blobs:
            assert rc[r] == full[blobs[r]][0] and rp[r] == full[blobs[r]][1]


def test_only_invalid_rows_and_empty_call(hip, full):
    rows = [(list(range(63)), [full[0][0][c] for c in range(63)])] * 2
    ret, craw, praw, st = _raw_call(hip, rows)
    assert ret == 1 and st == [1, 1]
    assert craw == b"\xa5" * (2 * CELLS) and praw == b"\xa5" * (2 * PROOFS)
    ret, craw, praw, st = _raw_call(hip, [])
    assert ret == 0 and craw == b"\xa5" * CELLS and praw == b"\xa5" * PROOFS
    assert hip.recover_cells_and_kzg_proofs_rows([]) == ([], [], [])


def test_malformed_arguments_write_nothing(hip, full):
    rows = _mixed(full)[:2]
    n0, n1 = len(rows[0][0]), len(rows[1][0])
    for start in ([1, n0, n0 + n1], [0, n0 + n1, n0]):
        ret, craw, praw, st = _raw_call(hip, rows, start=start)
        assert ret == 1
        assert craw == b"\xa5" * (2 * CELLS) and praw == b"\xa5" * (2 * PROOFS) and st == [0xa5, 0xa5]
    ret, _, _, st = _raw_call(hip, rows, want_cells=False, want_proofs=False)   # no output requested
    assert ret == 1 and st == [0xa5, 0xa5]
    ret, craw, praw, st = _raw_call(hip, rows)
    assert ret == 0 and st == [0, 0]
    assert craw == b"".join(full[0][0]) + b"".join(full[1][0])


def test_uniform_rows_equal_the_batch_call(hip, full):
    sets = _sets()
    for name in ("random_70", "all_128"):
        keep = sets[name]
        per_row = [[full[b][0][c] for c in keep] for b in range(4)] * 3
        bc, bp = hip.recover_cells_and_kzg_proofs_batch(keep, per_row)
        rc, rp, st = hip.recover_cells_and_kzg_proofs_rows([(keep, cells) for cells in per_row])
        assert st == [0] * 12
        assert rc == bc and rp == bp


def test_rows_split_over_two_replicas(full):
    # (two table replicas on one GPU stand in for two devices: the same fan-out, and no second GPU is needed)
    sets = _sets()
    names = list(sets)
    rows, blobs = [], []
    for r in range(44):
        b, keep = (3 * r + 1) % 4, sets[names[(5 * r + r // 7) % 7]]
        rows.append((keep, [full[b][0][c] for c in keep]))
        blobs.append(b)
    rows[20] = (list(range(63)), rows[20][1][:63])   # an invalid row in the first shard
    rows[30] = (list(range(60)), rows[30][1][:60])   # and one in the second
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        rc, rp, st = api.recover_cells_and_kzg_proofs_rows(rows)
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)
    assert st == [int(r in (20, 30)) for r in range(44)]
    for r in range(44):
        if r in (20, 30):
            assert rc[r] is None and rp[r] is None
        else:
            assert rc[r] == full[blobs[r]][0] and rp[r] == full[blobs[r]][1], "row %d" % r


def test_concurrent_callers(hip, full):
    """eight threads, each with its own mix of rows (some over the piped size, some under), on one KZGSettings"""
    import threading
    sets = _sets()
    names = list(sets)
    calls = []
    for t in range(8):
        rows, blobs = [], []
        for r in range(3 + 4 * t):
            b, keep = (r + t) % 4, sets[names[(3 * r + t) % 7]]
            rows.append((keep, [full[b][0][c] for c in keep]))
            blobs.append(b)
        calls.append((rows, blobs))
    results, errors = [None] * 8, []

    def work(t):
        try:
            results[t] = hip.recover_cells_and_kzg_proofs_rows(calls[t][0])
        except Exception as e:   # noqa: BLE001 -- reported below, in the test's thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(8):
        rc, rp, st = results[t]
        assert st == [0] * len(calls[t][0])
        _expect_rows(full, calls[t][1], rc, rp)


def test_device_rows_shifted_against_caller_rows_across_the_chunk_edge(hip, full):
    """515 rows over three sets.  Row 1 holds 63 cells: it is invalid and gets no device row, so the first chunk of 512
    device rows ends at caller row 512 and from row 2 on device row and caller row differ.  Rows 512 (the last device
    row of the first chunk) and 513 (the first of the second) carry a field element >= r."""
    sets = _sets()
    names = ["random_70", "even", "last_64"]
    nr = 515
    blob_of = [(3 * r + r // 7) % 4 for r in range(nr)]
    keeps = [sets[names[(r + r // 5) % 3]] for r in range(nr)]
    rows = [(keep, [full[blob_of[r]][0][c] for c in keep]) for r, keep in enumerate(keeps)]
    rows[1] = (list(range(63)), [full[blob_of[1]][0][c] for c in range(63)])
    for r, at, elem in ((512, 0, 0), (513, 40, 17)):
        cell = bytearray(rows[r][1][at])
        cell[elem * 32:(elem + 1) * 32] = R.to_bytes(32, "big")
        rows[r][1][at] = bytes(cell)
    assert len({tuple(rows[r][0]) for r in (0, 2, 511, 514)}) == 3
    ret, craw, praw, st = _raw_call(hip, rows)
    assert ret == 1
    assert [r for r in range(nr) if st[r] != 0] == [1, 512, 513] and st[1] == st[512] == st[513] == 1
    assert craw[CELLS:2 * CELLS] == b"\xa5" * CELLS and praw[PROOFS:2 * PROOFS] == b"\xa5" * PROOFS
    for r in (0, 2, 511, 514):
        assert craw[r * CELLS:(r + 1) * CELLS] == b"".join(full[blob_of[r]][0]), "cells of row %d" % r
        assert praw[r * PROOFS:(r + 1) * PROOFS] == b"".join(full[blob_of[r]][1]), "proofs of row %d" % r


@pytest.mark.parametrize("name", ["random_70", "all_128"])
@pytest.mark.parametrize("nr", [8, 9])
def test_piped_boundary_every_output_form_both_calls(hip, full, nr, name):
    """8 rows are the last call that copies its outputs back directly, 9 the first that drains them through the pipe;
    all_128 at 9 rows is the piped path that skips the transforms and returns the scattered image.  The batch call
    and the rows call, each as cells + proofs, cells only and proofs only, give the full rows."""
    keep = _sets()[name]
    blobs = [(r + r // 4) % 4 for r in range(nr)]
    per_row = [[full[b][0][c] for c in keep] for b in blobs]
    want_c, want_p = [full[b][0] for b in blobs], [full[b][1] for b in blobs]
    for want_cells, want_proofs in ((True, True), (True, False), (False, True)):
        bc, bp = hip.recover_cells_and_kzg_proofs_batch(keep, per_row, want_cells, want_proofs)
        rc, rp, st = hip.recover_cells_and_kzg_proofs_rows([(keep, cells) for cells in per_row], want_cells, want_proofs)
        assert st == [0] * nr
        assert bc == rc == (want_c if want_cells else None)
        assert bp == rp == (want_p if want_proofs else None)
