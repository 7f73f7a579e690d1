"""GPU tests of ckzg_hip_repair_cosets_and_kzg_proofs_rows and ckzg_hip_repair_cells_and_kzg_proofs_rows: recovery by rows
from untrusted cosets -- one verdict a row from the degree check and the commitment check, and with the held cosets'
proofs the repair pass (locate, drop, recover again).  Expected values never come from the calls under test: true rows
and cell proofs are the oracle's compute_cells_and_kzg_proofs and blob_to_kzg_commitment, proofs at e < 6 are
ckzg_hip_compute_coset_kzg_proofs_batch of the blob (as tests/test_gpu_coset_recover.py takes them), and the outputs on
false input are the bytes of the existing unchecked rows call, at e = 6 also the oracle's recover_cells_and_kzg_proofs
on the same false input.  Everything is compared byte for byte."""
import ctypes as C
import json
import os
import pickle
import random
import sys

import pytest

from conftest import ROOT
from test_gpu_commitment import rand_blob
from test_gpu_coset_recover import CHUNK_ROWS, EVALS, R, cut, held_sets, raw_call
from watchdog import run_watched

pytestmark = pytest.mark.gpu
OK, INCONSISTENT, MISMATCH, REPAIRED, UNRECOVERABLE, INVALID = range(6)
COSETS, CELLS = "ckzg_hip_repair_cosets_and_kzg_proofs_rows", "ckzg_hip_repair_cells_and_kzg_proofs_rows"
ES = list(range(7))
A5 = 0xa5


@pytest.fixture(scope="module")
def full(oracle):
    """two random blobs: extended evaluations (the oracle's 128 cells back to back), cell proofs, commitment"""
    out = []
    for i in range(2):
        blob = rand_blob(97, i)
        cells, proofs = oracle.compute_cells_and_kzg_proofs(blob)
        ext = b"".join(cells)
        assert len(ext) == EVALS and ext[:len(blob)] == blob
        out.append(dict(blob=blob, ext=ext, cell_proofs=b"".join(proofs), cm=oracle.blob_to_kzg_commitment(blob)))
    return out


@pytest.fixture(scope="module")
def all_proofs(hip, full):
    """e -> per blob its m coset proofs back to back: the oracle's cell proofs at e = 6, the openings call below"""
    cache = {6: [f["cell_proofs"] for f in full]}

    def get(e):
        if e not in cache:
            proofs, status = hip.compute_coset_kzg_proofs_batch([f["blob"] for f in full], e)
            assert status == [0, 0]
            cache[e] = [b"".join(p) for p in proofs]
        return cache[e]
    return get


def bump(data, value_index):
    """data with its value_index-th 32-byte value replaced by value + 1 mod r"""
    at = 32 * value_index
    v = (int.from_bytes(data[at:at + 32], "big") + 1) % R
    return data[:at] + v.to_bytes(32, "big") + data[at + 32:]


def repair(api, rows, e, cms=None, proofs=None, want_evals=True, want_proofs=False, entry=COSETS, start=None,
           verdict=True, want_ok=None, status=True):
    """the C call over buffers filled with 0xA5.  rows: (indices, bytes); cms: a list of 48-byte strings; proofs: per row
    the held cosets' proofs back to back.  Returns a dict: ret, ev, pr, st, vd, ok (flat list), stats"""
    nr, ps = len(rows), 48 * (8192 >> min(e, 6))
    if start is None:
        start = [0]
        for idx, _ in rows:
            start.append(start[-1] + len(idx))
    flat = [i for idx, _ in rows for i in idx]
    f = getattr(api.lib, entry)
    f.restype = C.c_int
    fill = lambda n: (C.c_char * n).from_buffer(bytearray([A5]) * n)
    rv = fill(max(nr, 1) * EVALS) if want_evals else None
    rp = fill(max(nr, 1) * ps) if want_proofs else None
    st = (C.c_uint8 * max(nr, 1))(*([A5] * max(nr, 1))) if status else None
    vd = (C.c_uint8 * max(nr, 1))(*([A5] * max(nr, 1))) if verdict else None
    if want_ok is None:
        want_ok = proofs is not None
    ok = (C.c_uint8 * max(len(flat), 1))(*([A5] * max(len(flat), 1))) if want_ok else None
    stats = (C.c_uint64 * 4)(*([A5] * 4))
    args = [rv, rp, st, vd, ok, stats, (C.c_uint64 * max(len(flat), 1))(*flat), b"".join(b for _, b in rows),
            (C.c_uint64 * len(start))(*start), C.c_uint64(nr), b"".join(cms) if cms is not None else None,
            b"".join(proofs) if proofs is not None else None]
    if entry == COSETS:
        args.append(C.c_uint32(e))
    ret = f(*args, api.sp)
    return dict(ret=ret, ev=rv.raw if want_evals else None, pr=rp.raw if want_proofs else None,
                st=list(st)[:nr] if status else None, vd=list(vd)[:nr] if verdict else None,
                ok=list(ok)[:len(flat)] if want_ok else None, stats=list(stats))


def row_of(out, r, e, what="ev"):
    size = EVALS if what == "ev" else 48 * (8192 >> e)
    return out[what][r * size:(r + 1) * size]


# ---- everything true ----

@pytest.mark.parametrize("e", ES)
def test_true_rows_are_ok_and_the_oracles_bytes(hip, full, e):
    sets = held_sets(e)
    names = list(sets)
    assert len(names) == 8
    blobs = [r % 2 for r in range(len(names))]
    rows = [(sets[n], cut(full[b]["ext"], sets[n], e)) for n, b in zip(names, blobs)]
    out = repair(hip, rows, e, [full[b]["cm"] for b in blobs])
    assert out["ret"] == 0 and out["st"] == [0] * 8
    assert out["vd"] == [OK] * 8, dict(zip(names, out["vd"]))
    for r, b in enumerate(blobs):
        assert row_of(out, r, e) == full[b]["ext"], "row %d (%s)" % (r, names[r])
    assert out["stats"] == [0] * 4     # no proofs given: nothing goes to repair
    none = repair(hip, rows, e, None)
    assert none["ret"] == 0 and none["vd"] == [OK] * 8 and none["ev"] == out["ev"]


# ---- verdicts; the outputs are the unchecked call's ----

def verdict_rows(full, e):
    """(name, row, blob of the commitment given or bytes, expected verdict with commitments, without)"""
    m, l = 8192 >> e, 1 << e
    sets = held_sets(e)
    ext = [f["ext"] for f in full]
    over = sets["half_less_one_missing"]       # m / 2 + 1 cosets
    half = sets["random_half"]                 # exactly m / 2
    everything = sets["all"]
    assert len(over) == m // 2 + 1 and len(half) == m // 2
    junk = lambda idx: (idx, bytes((32 << e) * len(idx)))
    good_half = cut(ext[1], half, e)
    non_canonical = good_half[:32 * 7] + R.to_bytes(32, "big") + good_half[32 * 8:]
    not_g1 = b"\xff" * 48
    return [
        ("over_half_one_changed", (over, bump(cut(ext[0], over, e), 3 * l + l - 1)), 0, INCONSISTENT, INCONSISTENT),
        ("half_one_changed", (half, bump(cut(ext[1], half, e), (m // 2 - 1) * l)), 1, MISMATCH, OK),
        ("good", (sets["even_missing"], cut(ext[0], sets["even_missing"], e)), 0, OK, OK),
        ("full_changed_in_extension", (everything, bump(ext[0], 4096 + 17)), 0, INCONSISTENT, INCONSISTENT),
        ("full_changed_in_blob", (everything, bump(ext[1], 4095)), 1, INCONSISTENT, INCONSISTENT),
        ("too_few", junk(list(range(m // 2 - 1))), 0, INVALID, INVALID),
        ("true_row_other_commitment", (sets["one_missing"], cut(ext[0], sets["one_missing"], e)), 1, MISMATCH, OK),
        ("non_canonical", (half, non_canonical), 1, INVALID, INVALID),
        ("commitment_not_g1", (sets["first_half_missing"], cut(ext[1], sets["first_half_missing"], e)), not_g1, MISMATCH, OK),
        ("good_again", (half, good_half), 1, OK, OK),
    ]


@pytest.mark.parametrize("e", [0, 3, 6])
def test_verdicts_and_outputs_equal_the_unchecked_call(hip, oracle, full, e):
    cases = verdict_rows(full, e)
    names = [c[0] for c in cases]
    rows = [c[1] for c in cases]
    cms = [full[c[2]]["cm"] if isinstance(c[2], int) else c[2] for c in cases]
    # the extension-half case: the row's first 4096 values still commit to the given commitment
    ext_case = rows[names.index("full_changed_in_extension")][1]
    assert ext_case[:4096 * 32] == full[0]["blob"] and oracle.blob_to_kzg_commitment(ext_case[:4096 * 32]) == full[0]["cm"]
    ret0, ev0, pr0, st0 = raw_call(hip, rows, e)                     # the existing call on the same input
    assert ret0 == 1 and st0 == [1 if c[3] == INVALID else 0 for c in cases]
    out = repair(hip, rows, e, cms, want_proofs=True)
    assert out["ret"] == ret0 and out["st"] == st0
    assert out["vd"] == [c[3] for c in cases], dict(zip(names, out["vd"]))
    assert out["ev"] == ev0 and out["pr"] == pr0
    none = repair(hip, rows, e, None, want_proofs=True)
    assert none["ret"] == ret0 and none["st"] == st0
    assert none["vd"] == [c[4] for c in cases], dict(zip(names, none["vd"]))
    assert none["ev"] == ev0 and none["pr"] == pr0
    # the neighbours of the invalid rows are unaffected; the invalid ones keep the sentinel
    assert row_of(out, names.index("good"), e) == full[0]["ext"] and row_of(out, names.index("good_again"), e) == full[1]["ext"]
    assert row_of(out, names.index("too_few"), e) == bytes([A5]) * EVALS
    if e == 6:   # ... and the oracle's recovery of the same false input
        for name in ("over_half_one_changed", "half_one_changed"):
            r = names.index(name)
            idx, data = rows[r]
            ec, ep = oracle.recover_cells_and_kzg_proofs(idx, [data[2048 * i:2048 * (i + 1)] for i in range(len(idx))])
            assert row_of(out, r, e) == b"".join(ec) and row_of(out, r, e, "pr") == b"".join(ep), name
            assert b"".join(ec) != full[cases[r][2]]["ext"]


@pytest.mark.parametrize("e", [2, 6])
def test_a_chunk_of_full_rows_only(hip, full, e):
    """every row holds all m cosets: the unchecked call transforms nothing there, the checks still see the coefficients"""
    everything = list(range(8192 >> e))
    rows = [(everything, full[0]["ext"]), (everything, bump(full[0]["ext"], 8191)), (everything, bump(full[1]["ext"], 0)),
            (everything, full[1]["ext"]), (everything, full[1]["ext"])]
    cms = [full[b]["cm"] for b in (0, 0, 1, 1, 0)]
    ret0, ev0, pr0, st0 = raw_call(hip, rows, e, True, e == 6)
    out = repair(hip, rows, e, cms, want_proofs=e == 6)
    assert (out["ret"], out["st"]) == (ret0, st0) == (0, [0] * 5)
    assert out["vd"] == [OK, INCONSISTENT, INCONSISTENT, OK, MISMATCH]
    assert out["ev"] == ev0 == b"".join(d for _, d in rows) and out["pr"] == pr0


# ---- repair ----

def held_proofs(proofs_of_blob, idx):
    return b"".join(proofs_of_blob[48 * c:48 * c + 48] for c in idx)


@pytest.mark.parametrize("e", [0, 3, 6])
def test_repair_drops_false_cosets_and_recovers_from_the_rest(hip, full, all_proofs, e):
    m, l = 8192 >> e, 1 << e
    rnd = random.Random(60 + e)
    pr = all_proofs(e)
    sets = held_sets(e)
    plus3 = [sorted(rnd.sample(range(m), m // 2 + 3)) for _ in range(2)]
    half = sets["random_half"]
    rows, cms, hp, blobs = [], [], [], [0, 1, 1, 0, 1]
    # row 0: m / 2 + 3 cosets, two of them false
    false0 = sorted(rnd.sample(range(m // 2 + 3), 2))
    data = cut(full[0]["ext"], plus3[0], e)
    for j in false0:
        data = bump(data, j * l + rnd.randrange(l))
    rows.append((plus3[0], data)), hp.append(held_proofs(pr[0], plus3[0]))
    # row 1: a true row
    rows.append((sets["even_missing"], cut(full[1]["ext"], sets["even_missing"], e))), hp.append(held_proofs(pr[1], sets["even_missing"]))
    # row 2: exactly m / 2 cosets, one false
    false2 = rnd.randrange(m // 2)
    rows.append((half, bump(cut(full[1]["ext"], half, e), false2 * l))), hp.append(held_proofs(pr[1], half))
    # row 3: m / 2 + 3 cosets, one false value and a false proof on a true coset (the proof of another coset)
    false3, badproof3 = 5, m // 2
    data = bump(cut(full[0]["ext"], plus3[1], e), false3 * l + l - 1)
    p3 = bytearray(held_proofs(pr[0], plus3[1]))
    p3[48 * badproof3:48 * badproof3 + 48] = p3[48 * (badproof3 + 1):48 * (badproof3 + 2)]
    rows.append((plus3[1], data)), hp.append(bytes(p3))
    # row 4: a true full row
    rows.append((sets["all"], full[1]["ext"])), hp.append(pr[1])
    cms = [full[b]["cm"] for b in blobs]
    out = repair(hip, rows, e, cms, hp, want_proofs=True)
    assert out["ret"] == 0 and out["st"] == [0] * 5
    assert out["vd"] == [REPAIRED, OK, UNRECOVERABLE, REPAIRED, OK]
    start = [0]
    for idx, _ in rows:
        start.append(start[-1] + len(idx))
    ok = [out["ok"][start[r]:start[r + 1]] for r in range(5)]
    assert all(v in (0, 1) for v in out["ok"])
    assert [j for j, v in enumerate(ok[0]) if not v] == false0
    assert ok[1] == [1] * len(rows[1][0]) and ok[4] == [1] * m
    assert [j for j, v in enumerate(ok[2]) if not v] == [false2]
    assert [j for j, v in enumerate(ok[3]) if not v] == [false3, badproof3]
    for r in (0, 1, 3, 4):
        assert row_of(out, r, e) == full[blobs[r]]["ext"], "evaluations of row %d" % r
        assert row_of(out, r, e, "pr") == pr[blobs[r]], "proofs of row %d" % r
    # the true rows spend no locate work
    assert out["stats"][:3] == [3, len(rows[0][0]) + len(rows[2][0]) + len(rows[3][0]), 2] and out["stats"][3] >= 1


# ---- boundaries ----

def test_nine_rows_where_the_piped_output_path_begins(hip, full, all_proofs):
    e, m, l = 4, 512, 16
    sets = held_sets(e)
    names = ["random_half", "odd_count_missing", "all"]
    pick = [((r + r // 4) % 2, names[r % 3]) for r in range(9)]
    rows = [(sets[n], cut(full[b]["ext"], sets[n], e)) for b, n in pick]
    rows[4] = (rows[4][0], bump(rows[4][1], 100))      # odd_count_missing, one value changed: inconsistent
    rows[8] = (rows[8][0], bump(rows[8][1], 8000))     # a full row
    pr = all_proofs(e)
    hp = [held_proofs(pr[b], sets[n]) for b, n in pick]
    ret0, ev0, pr0, st0 = raw_call(hip, rows, e)
    first = repair(hip, rows, e, [full[b]["cm"] for b, _ in pick], want_proofs=True)
    want = [OK] * 9
    want[4] = want[8] = INCONSISTENT
    assert first["ret"] == ret0 == 0 and first["vd"] == want and first["ev"] == ev0 and first["pr"] == pr0
    out = repair(hip, rows, e, [full[b]["cm"] for b, _ in pick], hp, want_proofs=True)
    want[4] = want[8] = REPAIRED
    assert out["ret"] == 0 and out["vd"] == want and out["stats"][:3] == [2, len(rows[4][0]) + m, 2]
    for r, (b, _) in enumerate(pick):
        assert row_of(out, r, e) == full[b]["ext"] and row_of(out, r, e, "pr") == pr[b], "row %d" % r


def test_more_rows_than_a_chunk_and_the_cell_entry(hip, full):
    """129 rows at e = 6, evaluations only: the coset entry's chunk is 128 rows; false rows at 127 and 128.  The cell
    entry, whose chunk is 512 rows, gives the same verdicts and bytes."""
    e = 6
    assert CHUNK_ROWS == 128
    sets = held_sets(e)
    names = ["random_half", "even_missing", "half_less_one_missing", "all"]
    pieces = {(b, n): cut(full[b]["ext"], sets[n], e) for b in range(2) for n in names}
    pick = [((r + r // 3) % 2, names[(r + r // 7) % 4]) for r in range(129)]
    pick[127] = (0, "half_less_one_missing")
    pick[128] = (1, "random_half")
    rows = [(sets[n], pieces[(b, n)]) for b, n in pick]
    rows[127] = (rows[127][0], bump(rows[127][1], 64 * 11 + 5))
    rows[128] = (rows[128][0], bump(rows[128][1], 64 * 63 + 63))
    cms = [full[b]["cm"] for b, _ in pick]
    want = [OK] * 129
    want[127], want[128] = INCONSISTENT, MISMATCH
    out = repair(hip, rows, e, cms)
    assert out["ret"] == 0 and out["st"] == [0] * 129 and out["vd"] == want
    for r, (b, _) in enumerate(pick):
        if r < 127:
            assert row_of(out, r, e) == full[b]["ext"], "row %d" % r
    ret0, ev0, _, st0 = raw_call(hip, rows[127:], e, True, False)
    assert ret0 == 0 and out["ev"][127 * EVALS:] == ev0
    cell = repair(hip, rows, e, cms, entry=CELLS)
    assert (cell["ret"], cell["st"], cell["vd"]) == (0, [0] * 129, want) and cell["ev"] == out["ev"]


# ---- check-only mode, rejected calls, the empty call ----

@pytest.mark.parametrize("e", [1, 6])
def test_check_only_mode(hip, full, all_proofs, e):
    m, l = 8192 >> e, 1 << e
    sets = held_sets(e)
    everything = sets["all"]
    rows = [(everything, full[0]["ext"]),                                     # a full row against its commitment: no proof at all
            (everything, bump(full[1]["ext"], 4096 + 4095)),
            (sets["random_half"], cut(full[1]["ext"], sets["random_half"], e)),
            (sets["random_half"], cut(full[1]["ext"], sets["random_half"], e))]
    cms = [full[0]["cm"], full[1]["cm"], full[1]["cm"], full[0]["cm"]]
    out = repair(hip, rows, e, cms, want_evals=False)
    assert out["ret"] == 0 and out["st"] == [0] * 4 and out["vd"] == [OK, INCONSISTENT, OK, MISMATCH]
    if e == 6:   # ... and repair without outputs: the verdicts and coset_ok alone
        hp = [all_proofs(e)[b] if len(idx) == m else held_proofs(all_proofs(e)[b], idx) for (idx, _), b in zip(rows, (0, 1, 1, 1))]
        out = repair(hip, rows, e, cms, hp, want_evals=False)
        assert out["vd"] == [OK, REPAIRED, OK, UNRECOVERABLE] and out["stats"][:3] == [2, m + m // 2, 1]
        assert out["ok"][:m] == [1] * m and out["ok"][m:2 * m] == [1] * (m - 1) + [0]
        assert out["ok"][2 * m:2 * m + m // 2] == [1] * (m // 2) and out["ok"][2 * m + m // 2:] == [0] * (m // 2)


def test_rejected_calls_leave_every_buffer_untouched(hip, full):
    e = 5
    idx = held_sets(e)["random_half"]
    rows = [(idx, cut(full[0]["ext"], idx, e))] * 2
    cms = [full[0]["cm"]] * 2
    hp = [bytes(48 * len(idx))] * 2
    n = len(idx)
    untouched = lambda o: (o["ev"] == bytes([A5]) * len(o["ev"]) and o["pr"] == bytes([A5]) * len(o["pr"]) and o["st"] == [A5, A5]
                           and (o["vd"] is None or o["vd"] == [A5, A5]) and (o["ok"] is None or o["ok"] == [A5] * (2 * n))
                           and o["stats"] == [A5] * 4)
    for kw in (dict(cms=None, proofs=hp),                          # proofs without commitments
               dict(cms=cms, proofs=None, want_ok=True),           # coset_ok without proofs
               dict(cms=cms, verdict=False),                       # no verdict
               dict(cms=cms, start=[1, n, 2 * n]), dict(cms=cms, start=[0, 2 * n, n])):
        out = repair(hip, rows, e, want_proofs=True, **kw)
        assert out["ret"] == 1 and untouched(out), kw
    out = repair(hip, rows, 7, cms, want_proofs=True)
    assert out["ret"] == 1 and untouched(out)
    f = getattr(hip.lib, COSETS)
    f.restype = C.c_int
    vd = (C.c_uint8 * 1)(A5)
    start = (C.c_uint64 * 2)(0, n)
    assert f(None, None, None, vd, None, None, None, None, start, C.c_uint64(1), None, None, C.c_uint32(e), hip.sp) == 1
    assert list(vd) == [A5]                                        # NULL inputs with work to do
    # the empty call
    assert f(None, None, None, None, None, None, None, None, None, C.c_uint64(0), None, None, C.c_uint32(e), hip.sp) == 0
    g = getattr(hip.lib, CELLS)
    g.restype = C.c_int
    assert g(None, None, None, None, None, None, None, None, None, C.c_uint64(0), None, None, hip.sp) == 0


def test_the_binding(hip, full, all_proofs):
    e = 6
    idx = sorted(random.Random(9).sample(range(128), 67))
    data = bump(cut(full[0]["ext"], idx, e), 64 * 2)
    ev, pr, st, vd, ok, stats = hip.repair_cosets_and_kzg_proofs_rows(
        [(idx, data)], e, [full[0]["cm"]], [[all_proofs(e)[0][48 * c:48 * c + 48] for c in idx]])
    assert st == [0] and vd == [REPAIRED] and ok == [[j != 2 for j in range(67)]] and stats[:3] == [1, 67, 1]
    assert ev == [full[0]["ext"]] and pr == [all_proofs(e)[0]]


# ---- on poisoned temporaries, in a child process ----

def test_on_poisoned_temporaries(oracle, full, all_proofs, tmp_path):
    """tests/coset_repair_poison_driver.py: one small repair call at e = 3 and e = 6 with option "poison_temporaries" off,
    0xFF and 0x01, each on settings loaded for that run; what it returns must be the same in all three and what the
    oracle says"""
    cases = {}
    for e in (3, 6):
        m, l = 8192 >> e, 1 << e
        rnd = random.Random(80 + e)
        sets = held_sets(e)
        idx = sorted(rnd.sample(range(m), m // 2 + 3))
        pr = all_proofs(e)
        rows = [(idx, bump(bump(cut(full[0]["ext"], idx, e), 2 * l), 9 * l + 1)),
                (sets["random_half"], cut(full[1]["ext"], sets["random_half"], e)),
                (sets["random_half"], bump(cut(full[1]["ext"], sets["random_half"], e), 0)),
                (sets["all"], full[0]["ext"])]
        blobs = [0, 1, 1, 0]
        cases[e] = dict(rows=rows, cms=[full[b]["cm"] for b in blobs],
                        hp=[held_proofs(pr[b], ix) for (ix, _), b in zip(rows, blobs)],
                        want=dict(vd=[REPAIRED, OK, UNRECOVERABLE, OK], st=[0] * 4,
                                  ev={0: full[0]["ext"], 1: full[1]["ext"], 3: full[0]["ext"]},
                                  pr={0: pr[0], 1: pr[1], 3: pr[0]},
                                  bad_ok=[2, 9, len(idx) + m // 2], stats=[2, len(idx) + m // 2, 1]))
    case_path, report_path = str(tmp_path / "cases.pickle"), str(tmp_path / "report.json")
    with open(case_path, "wb") as f:
        pickle.dump(cases, f)
    # three loads of small tables and six small calls: 1.5 s measured with the fill off in all three runs, times four
    res = run_watched([sys.executable, os.path.join(ROOT, "tests", "coset_repair_poison_driver.py"), case_path, report_path],
                      timeout=8, name="poison_coset_repair")
    assert os.path.exists(report_path), "no report:\n" + res.stderr[-3000:]
    report = json.load(open(report_path))
    print("poison coset_repair: seconds per run %s" % report["seconds"])
    assert report["stopped"] is None, "%s\n%s" % (report["stopped"], res.stderr[-3000:])
    assert res.returncode == 0 and report["done"], res.stderr[-3000:]
    assert list(report["runs"]) == ["0x00", "0xFF", "0x01"]
    wrong = ["fill %s, e = %s: %s" % (fill, e, what) for fill, run in report["runs"].items() for e, fails in run.items() for what in fails]
    assert not wrong, "\n".join(wrong)
    assert report["digests"]["0x00"] == report["digests"]["0xFF"] == report["digests"]["0x01"]
