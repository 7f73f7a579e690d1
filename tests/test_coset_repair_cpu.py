"""ckzg_hip_repair_cosets_and_kzg_proofs_rows / ckzg_hip_repair_cells_and_kzg_proofs_rows without a GPU: the symbols are
declared, exported and bound, the verdict values of the header are those of the plan, a settings struct without GPU
state gives C_KZG_ERROR (no CPU fallback), and the repair planning the product runs (csrc/coset_repair_plan.hpp, through
libhost_shim.so) agrees with the model (tests/coset_repair_expect.py) at e = 0, 3, 6: rows to locate and their item
arrays, filtering with the threshold at exactly m / 2, second-pass row placement, verdict precedence."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import coset_repair_expect as X
from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, Kzg, KzgError, KZGSettings
from test_abi_exports import declared_symbols

NAMES = ["ckzg_hip_repair_cosets_and_kzg_proofs_rows", "ckzg_hip_repair_cells_and_kzg_proofs_rows"]


def test_symbols_declared_exported_and_bound():
    exports = open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    lib = C.CDLL(HIP_SO)
    for name in NAMES:
        assert name in declared_symbols()
        assert "    %s;\n" % name in exports
        assert hasattr(lib, name)
    assert callable(getattr(Kzg, "repair_cosets_and_kzg_proofs_rows"))


def test_header_verdicts_are_the_models():
    header = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    for value, name in enumerate(X.NAMES):
        assert re.search(r"#define CKZG_HIP_ROW_%s\s+%d\b" % (name, value), header), name


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    lib = C.CDLL(HIP_SO)
    s = KZGSettings()
    f = getattr(lib, NAMES[0])
    f.restype = C.c_int
    vd = (C.c_uint8 * 1)(0xa5)
    idx = (C.c_uint64 * 64)(*range(64))
    start = (C.c_uint64 * 2)(0, 64)
    assert f(None, None, None, vd, None, None, idx, bytes(64 * 2048), start, C.c_uint64(1), None, None, C.c_uint32(6), C.byref(s)) == 2
    assert f(None, None, None, vd, None, None, idx, bytes(64 * 2048), start, C.c_uint64(1), None, None, C.c_uint32(7), C.byref(s)) == 1
    g = getattr(lib, NAMES[1])
    g.restype = C.c_int
    assert g(None, None, None, vd, None, None, idx, bytes(64 * 2048), start, C.c_uint64(1), None, None, C.byref(s)) == 2
    assert list(vd) == [0xa5]


def test_binding_checks_its_arguments():
    api = Kzg.__new__(Kzg)   # no library: every check below fails before a call is made
    item = bytes(32 << 3)
    for kw in (dict(held_proofs=[[bytes(48)]]),                                  # proofs without commitments
               dict(commitments=[bytes(48)] * 2),                                # one commitment too many
               dict(commitments=[bytes(47)]),
               dict(commitments=[bytes(48)], held_proofs=[[bytes(48)] * 2]),     # two proofs for one coset
               dict(commitments=[bytes(48)], held_proofs=[[bytes(49)]])):
        with pytest.raises(KzgError):
            api.repair_cosets_and_kzg_proofs_rows([([0], item)], 3, **kw)
    with pytest.raises(KzgError):
        api.repair_cosets_and_kzg_proofs_rows([([0], item)], 7)


# ---- the plan ----

@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    lib.hs_coset_repair_plan.restype = C.c_long
    return lib


def _plan(h, status, high1, mism1, row_start, e, with_proofs, item_ok, high2, mism2, want_ok=True):
    nr, total = len(status), row_start[-1]
    u8 = lambda v: (C.c_uint8 * max(len(v), 1))(*[1 if x else 0 for x in v])
    u64 = lambda n: (C.c_uint64 * max(n, 1))(*([0xa5a5] * max(n, 1)))
    verdict, coset_ok = (C.c_uint8 * nr)(*([0xa5] * nr)), (C.c_uint8 * max(total, 1))(*([0xa5] * max(total, 1)))
    loc, isrc, irow, orow, st2, src2, lost, counts = u64(nr), u64(total), u64(total), u64(nr), u64(nr + 1), u64(total), u64(nr), u64(5)
    ret = h.hs_coset_repair_plan(verdict, coset_ok if want_ok else None, loc, isrc, irow, orow, st2, src2, lost, counts,
                                 (C.c_uint8 * nr)(*status), u8(high1), u8(mism1), u8(item_ok), u8(high2), u8(mism2),
                                 (C.c_uint64 * (nr + 1))(*row_start), C.c_uint64(nr), int(with_proofs), e)
    assert ret == 0
    c = list(counts)
    return dict(verdict=list(verdict), coset_ok=[bool(v) for v in coset_ok[:total]] if want_ok else None,
                loc_rows=list(loc[:c[0]]), item_src=list(isrc[:c[1]]), item_row=list(irow[:c[1]]), out_row=list(orow[:c[2]]),
                start2=list(st2[:c[2] + 1]), src2=list(src2[:c[3]]), lost=list(lost[:c[4]]))


def _compare(h, e, status, high1, mism1, held, with_proofs, item_ok, high2, mism2):
    row_start = [0]
    for n in held:
        row_start.append(row_start[-1] + n)
    got = _plan(h, status, high1, mism1, row_start, e, with_proofs, item_ok, high2, mism2)
    want = X.plan(status, high1, mism1, row_start, e, with_proofs, item_ok, high2, mism2)
    for key in want:
        assert got[key] == want[key], (key, e)
    return got, row_start


def test_verdict_precedence_every_combination(h):
    """invalid x high x mismatch, no proofs: INVALID, then INCONSISTENT, then MISMATCH, then OK; coset_ok follows OK"""
    combos = [(i, hi, mi) for i in (0, 1) for hi in (0, 1) for mi in (0, 1)]
    got, _ = _compare(h, 6, [c[0] for c in combos], [c[1] for c in combos], [c[2] for c in combos], [64] * 8, False,
                      [0] * 512, [0] * 8, [0] * 8)
    assert got["verdict"] == [X.OK, X.MISMATCH, X.INCONSISTENT, X.INCONSISTENT] + [X.INVALID] * 4
    assert got["coset_ok"] == [True] * 64 + [False] * (7 * 64)
    assert got["loc_rows"] == [] and got["start2"] == [0]
    # status is C_KZG_RET: any non-zero value is invalid
    got, _ = _compare(h, 6, [3, 0], [0, 0], [0, 0], [64, 64], False, [0] * 128, [0, 0], [0, 0])
    assert got["verdict"] == [X.INVALID, X.OK]


@pytest.mark.parametrize("e", [0, 3, 6])
def test_threshold_at_exactly_half(h, e):
    """rows of m / 2 + 2 cosets with 1, 2 and 3 false ones: m / 2 + 1, m / 2 (still recovered) and m / 2 - 1 (lost) remain"""
    m = 8192 >> e
    n = m // 2 + 2
    held = [n, n, n, n]
    item_ok = [1] * (4 * n)
    for row, bad in ((0, [5]), (1, [0, n - 1]), (2, [1, 2, n - 1])):
        for j in bad:
            item_ok[row * n + j] = 0
    # row 3 is fine in the first pass: it is not located, whatever item_ok says there
    item_ok[3 * n + 7] = 0
    got, row_start = _compare(h, e, [0] * 4, [1, 1, 0, 0], [0, 1, 1, 0], held, True, item_ok, [0] * 4, [0] * 4)
    assert got["loc_rows"] == [0, 1, 2] and got["lost"] == [2] and got["out_row"] == [0, 1]
    assert got["start2"] == [0, n - 1, 2 * n - 3]
    assert got["verdict"] == [X.REPAIRED, X.REPAIRED, X.UNRECOVERABLE, X.OK]
    assert got["item_src"] == list(range(3 * n)) and got["item_row"] == [0] * n + [1] * n + [2] * n
    assert got["src2"] == [i for i in range(2 * n) if item_ok[i]]
    assert got["coset_ok"] == [bool(v) for v in item_ok[:3 * n]] + [True] * n


@pytest.mark.parametrize("e", [0, 3, 6])
def test_random_calls_agree_with_the_model(h, e):
    m = 8192 >> e
    rnd = random.Random(700 + e)
    for trial in range(6 if e else 2):
        nr = rnd.randrange(1, 12)
        held = [rnd.choice([m // 2, m // 2 + 1, m // 2 + 3, m, rnd.randrange(m // 2, m + 1)]) for _ in range(nr)]
        status = [rnd.choice([0, 0, 0, 1]) for _ in range(nr)]
        flags = lambda p: [1 if rnd.random() < p else 0 for _ in range(nr)]
        total = sum(held)
        style = rnd.choice(["few", "many", "all"])
        p_bad = {"few": 2.0 / m, "many": 0.5, "all": 1.0}[style]
        item_ok = [0 if rnd.random() < p_bad else 1 for _ in range(total)]
        _compare(h, e, status, flags(0.4), flags(0.4), held, trial % 3 != 0, item_ok, flags(0.2), flags(0.2))


def test_second_pass_rows_land_at_their_caller_rows(h):
    """located rows are scattered among OK and INVALID ones: out_row names their caller rows in order, start2 cuts src2"""
    e, m = 3, 1024
    held = [m // 2 + 3] * 7
    n = held[0]
    status = [0, 0, 1, 0, 0, 0, 0]
    high1 = [0, 1, 1, 0, 1, 0, 0]
    mism1 = [0, 0, 0, 0, 0, 1, 0]
    item_ok = [1] * (7 * n)
    item_ok[1 * n + 4] = item_ok[1 * n + 9] = 0          # row 1: two false
    item_ok[5 * n] = 0                                   # row 5: one false
    for j in range(4):
        item_ok[4 * n + j] = 0                           # row 4: four false, one too many
    high2 = [0] * 7
    mism2 = [0, 0, 0, 0, 0, 1, 0]                        # row 5 still does not match after the second pass
    got, _ = _compare(h, e, status, high1, mism1, held, True, item_ok, high2, mism2)
    assert got["loc_rows"] == [1, 4, 5] and got["out_row"] == [1, 5] and got["lost"] == [4]
    assert got["start2"] == [0, n - 2, 2 * n - 3]
    assert got["verdict"] == [X.OK, X.REPAIRED, X.INVALID, X.OK, X.UNRECOVERABLE, X.UNRECOVERABLE, X.OK]
    assert got["src2"][:3] == [n, n + 1, n + 2] and got["src2"][n - 2] == 5 * n + 1
    # without a coset_ok array the plan is the same
    row_start = [i * n for i in range(8)]
    assert _plan(h, status, high1, mism1, row_start, e, True, item_ok, high2, mism2, want_ok=False)["verdict"] == got["verdict"]


def test_malformed_row_start_and_coset_size(h):
    z8, z64 = (C.c_uint8 * 4)(), (C.c_uint64 * 8)()
    args = lambda start, e: (z8, None, z64, z64, z64, z64, z64, z64, z64, z64, z8, z8, z8, z8, z8, z8,
                             (C.c_uint64 * 3)(*start), C.c_uint64(2), 0, e)
    assert h.hs_coset_repair_plan(*args([0, 1, 2], 7)) == -1
    assert h.hs_coset_repair_plan(*args([1, 1, 2], 6)) == -1
    assert h.hs_coset_repair_plan(*args([0, 2, 1], 6)) == -1
    assert h.hs_coset_repair_plan(*args([0, 1, 2], 6)) == 0
