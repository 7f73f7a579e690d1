"""ckzg_hip_recover_cosets_and_kzg_proofs_rows without a GPU: the symbol is declared, exported and bound, a settings
struct without GPU state gives C_KZG_ERROR (no CPU fallback), the binding checks its arguments, the index maps the
product builds (csrc/coset_recover_plan.hpp, through libhost_shim.so) agree with the model (tests/coset_recover_expect.py)
at e = 0, 3, 6, the picker and its slices have the properties the kernel relies on, and the factors of
csrc/coset_recover_factors.hpp -- the function the kernel calls, replayed on the host with every `parts` the picker can
return -- are the two products computed with Python integers and the closed forms of the two half sets."""
import ctypes as C
import os
import random
import subprocess

import pytest

import coset_recover_expect as X
from coset_recover_expect import NONE, R
from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, Kzg, KzgError, KZGSettings
from test_abi_exports import declared_symbols

NAME = "ckzg_hip_recover_cosets_and_kzg_proofs_rows"
ES = list(range(7))


def test_symbol_declared_exported_and_bound():
    assert NAME in declared_symbols()
    assert "    %s;\n" % NAME in open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    assert hasattr(C.CDLL(HIP_SO), NAME)
    assert callable(getattr(Kzg, "recover_cosets_and_kzg_proofs_rows"))
    header = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    assert "#define CKZG_HIP_COSET_RECOVER_CHUNK_ROWS " in header


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    f = getattr(C.CDLL(HIP_SO), NAME)
    f.restype = C.c_int
    s = KZGSettings()
    for e in (0, 6):
        m, item = 8192 >> e, 32 << e
        rv, rp, st = C.create_string_buffer(8192 * 32), C.create_string_buffer(m * 48), (C.c_uint8 * 1)()
        idx = (C.c_uint64 * (m // 2))(*range(m // 2))
        start = (C.c_uint64 * 2)(0, m // 2)
        assert f(rv, rp, st, idx, bytes(m // 2 * item), start, C.c_uint64(1), C.c_uint32(e), C.byref(s)) == 2
        assert f(None, None, None, None, None, None, C.c_uint64(0), C.c_uint32(e), C.byref(s)) == 2
        assert rv.raw == bytes(8192 * 32) and rp.raw == bytes(m * 48)
    # a coset size the library does not have is rejected whatever else is passed
    assert f(None, None, None, None, None, None, C.c_uint64(0), C.c_uint32(7), C.byref(s)) == 1


def test_binding_checks_its_arguments():
    api = Kzg.__new__(Kzg)   # no library: every check below fails before a call is made
    for e in (0, 3, 6):
        item = bytes(32 << e)
        for rows in ([([0], item, item)],                     # not a pair
                     [([0, 1], item)],                        # one item for two indices
                     [([0], item[:-1])],                      # short
                     [([0], item + b"0")],                    # long
                     [([-1], item)],                          # an index that is no uint64
                     [([1 << 64], item)],
                     [([0.5], item)]):
            with pytest.raises(KzgError):
                api.recover_cosets_and_kzg_proofs_rows(rows, e)
        with pytest.raises(KzgError):
            api.recover_cosets_and_kzg_proofs_rows([([0], item)], e, False, False)
    for e in (-1, 7, 1 << 32, 2.0):
        with pytest.raises(KzgError):
            api.recover_cosets_and_kzg_proofs_rows([([0], bytes(32))], e)


# ---- the plan ----

@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    for fn in ("hs_coset_recover_plan", "hs_coset_recover_plan_set"):
        getattr(lib, fn).restype = C.c_long
    for fn in ("hs_coset_recover_parts", "hs_coset_recover_block", "hs_coset_recover_slice_len", "hs_coset_recover_slice_valid"):
        getattr(lib, fn).restype = C.c_uint32
    lib.hs_coset_recover_factors.restype = None
    return lib


def _plan(h, rows, e, chunk_rows, start=None):
    nr, w = len(rows), (8192 >> e) // 32
    if start is None:
        start = [0]
        for r in rows:
            start.append(start[-1] + len(r))
    flat = [c for r in rows for c in r]
    n = max(len(flat), 1)
    valid = (C.c_uint8 * max(nr, 1))()
    per_row = [(C.c_uint32 * max(nr, 1))() for _ in range(3)]
    mask = (C.c_uint32 * (w * max(nr, 1)))()
    pos, dst = (C.c_uint32 * n)(), (C.c_uint32 * n)()
    cap = nr + 1
    info = (C.c_uint32 * (5 * cap))()
    idx, st = (C.c_uint64 * n)(*flat), (C.c_uint64 * len(start))(*start)
    ret = h.hs_coset_recover_plan(valid, per_row[0], per_row[1], per_row[2], mask, pos, dst, info, C.c_size_t(cap), idx, st,
                                  C.c_uint64(nr), C.c_int(e), C.c_size_t(chunk_rows))

    def of_set(chunk, s):
        miss, runs, nruns = (C.c_uint32 * 8192)(), (C.c_uint64 * (4 * cap))(), C.c_uint32(0)
        k = h.hs_coset_recover_plan_set(miss, C.c_size_t(8192), runs, C.c_size_t(cap), C.byref(nruns), idx, st, C.c_uint64(nr),
                                        C.c_int(e), C.c_size_t(chunk_rows), C.c_size_t(chunk), C.c_size_t(s))
        return k, list(miss[:max(k, 0)]), [tuple(runs[4 * i:4 * i + 4]) for i in range(nruns.value)]

    return dict(ret=ret, valid=list(valid)[:nr], chunk=list(per_row[0])[:nr], dev=list(per_row[1])[:nr],
                set=list(per_row[2])[:nr], mask=[tuple(mask[w * r:w * r + w]) for r in range(nr)], pos=list(pos),
                dst=list(dst), info=[tuple(info[5 * c:5 * c + 5]) for c in range(cap)], start=start, of_set=of_set)


def _mask_words(cols, e):
    v = sum(1 << c for c in cols)
    return tuple((v >> (32 * w)) & 0xffffffff for w in range((8192 >> e) // 32))


def _mixed_rows(e, seed):
    m = 8192 >> e
    rnd = random.Random(seed)
    h = m // 2
    last = list(range(h)) + [m - 2]          # two masks that differ only in the last word, and there in one bit
    last2 = list(range(h)) + [m - 1]
    sets = [list(range(0, m, 2)), list(range(h)), list(range(h, m)), sorted(rnd.sample(range(m), h)),
            sorted(rnd.sample(range(m), h + 6)), sorted(rnd.sample(range(m), m - 1)), list(range(m)), last, last2]
    good = [list(sets[i % len(sets)]) for i in range(20)]
    bad = [list(range(h - 1)),                                 # too few
           list(range(m)) + [m],                               # too many
           list(range(h - 1)) + [m],                           # an index = m
           list(range(h - 2)) + [h + 5, h + 4],                # descending
           list(range(h - 1)) + [h - 2],                       # a repeated index
           []]                                                 # an empty slice
    rows = [(r, True) for r in good] + [(r, False) for r in bad]
    rnd.shuffle(rows)
    return [r for r, _ in rows], [ok for _, ok in rows]


@pytest.mark.parametrize("e", [0, 3, 6])
@pytest.mark.parametrize("chunk_rows", [128, 5, 1])
def test_plan_agrees_with_the_model(h, e, chunk_rows):
    m = 8192 >> e
    rows, expect_valid = _mixed_rows(e, 11 + e)
    p = _plan(h, rows, e, chunk_rows)
    per_row, chunks = X.plan(rows, e, chunk_rows)
    assert [v is not None for v in per_row] == expect_valid
    assert p["ret"] == len(chunks) == (sum(expect_valid) + chunk_rows - 1) // chunk_rows
    assert p["valid"] == [int(v) for v in expect_valid]
    for r, want in enumerate(per_row):
        span = range(p["start"][r], p["start"][r + 1])
        if want is None:
            assert (p["chunk"][r], p["dev"][r], p["set"][r]) == (NONE, NONE, NONE)
            assert all(p["pos"][i] == NONE and p["dst"][i] == NONE for i in span)
            continue
        assert (p["chunk"][r], p["dev"][r], p["set"][r]) == want
        assert p["mask"][r] == _mask_words(rows[r], e)
        # every held coset lands at device row * m + c
        assert [p["dst"][i] for i in span] == [want[1] * m + c for c in rows[r]]
    for c, ch in enumerate(chunks):
        members = ch["rows"]
        assert len(members) <= chunk_rows                       # a chunk boundary never cuts a row: rows are whole
        pos = [p["pos"][i] for r in members for i in range(p["start"][r], p["start"][r + 1])]
        assert pos == list(range(len(pos)))                     # the device input is packed in caller order
        total_missing = sum(len(v) for v in ch["missing"])
        assert p["info"][c] == (len(members), len(pos), len(ch["sets"]), int(all(len(rows[r]) == m for r in members)),
                                total_missing)
        for s, held in enumerate(ch["sets"]):
            k, miss, runs = p["of_set"](c, s)
            assert k == m - len(held)
            # the root index l * brp(j), for the missing cosets only, ascending in j
            hs = set(held)
            assert miss == ch["missing"][s] == [X.brp(j, 13 - e) << e for j in range(m) if j not in hs]
            # runs are maximal: consecutive valid caller rows are one run, and no two runs touch
            assert runs == ch["runs"]
            for a, b in zip(runs, runs[1:]):
                between = range(a[0] + a[2], b[0])
                assert len(between) > 0 and all(per_row[r] is None for r in between)
        assert p["of_set"](c, len(ch["sets"]))[0] == -1
    # the two masks that differ only in their last word are two sets wherever they share a chunk
    for ch in chunks:
        tails = [s for s in ch["sets"] if len(s) == m // 2 + 1 and s[:m // 2] == tuple(range(m // 2)) and s[-1] >= m - 2]
        assert len(tails) == len(set(tails))


@pytest.mark.parametrize("e", [0, 3, 6])
def test_plan_all_full_empty_and_malformed(h, e):
    m = 8192 >> e
    p = _plan(h, [list(range(m))] * 3, e, 128)
    assert p["ret"] == 1 and p["info"][0] == (3, 3 * m, 1, 1, 0)
    assert _plan(h, [], e, 128)["ret"] == 0
    p = _plan(h, [list(range(10))], e, 128)
    assert p["ret"] == 0 and p["valid"] == [0]
    rows = [list(range(m // 2)), list(range(m // 2))]
    assert _plan(h, rows, e, 128, start=[1, m // 2, m])["ret"] == -1       # does not start at 0
    assert _plan(h, rows, e, 128, start=[0, m, m // 2])["ret"] == -1       # decreases
    assert _plan(h, rows, e, 128, start=[0, m // 2, m])["ret"] == 1
    assert _plan(h, rows, 7, 128)["ret"] == -1


# ---- the picker ----

def test_picker_and_slices(h):
    for e in ES:
        m = 8192 >> e
        seen = set()
        for sets in list(range(1, 40)) + [64, 128, 129, 256, 1024]:
            p = h.hs_coset_recover_parts(C.c_uint64(sets), C.c_int(e))
            assert p == X.parts(sets, e) and p & (p - 1) == 0 and p >= 1
            if sets * m // 64 >= X.FILL_WAVES:
                assert p == 1                                    # a full chip is not split
            seen.add(p)
            block = h.hs_coset_recover_block(C.c_int(e), C.c_uint32(p))
            assert block <= 256 and block % p == 0 and m % (block // p) == 0 and block == min(256, m * p)
        assert sorted(seen) == X.all_parts(e)
    for count in (0, 1, 3, 5, 31, 33, 63, 65, 1000, 4093, 4095, 4096):
        for p in (1, 2, 4, 8, 16, 32):
            step = h.hs_coset_recover_slice_len(C.c_uint32(count), C.c_uint32(p))
            got = []
            for q in range(p):
                v = h.hs_coset_recover_slice_valid(C.c_uint32(count), C.c_uint32(p), C.c_uint32(q))
                assert v <= step
                got.append((min(q * step, count), min(q * step, count) + v))
            assert got == X.slices(count, p)
            covered = [i for lo, hi in got for i in range(lo, hi)]
            assert covered == list(range(count))                 # exactly once, in order


# ---- the factors ----

@pytest.fixture(scope="module")
def roots_raw():
    return (C.c_uint32 * (8 * 8193))(*[w for v in X.roots() for w in X.limbs(v)])


def _replay(h, roots_raw, missing, which, e, parts):
    miss = [X.root_index(j, e) for j in missing]
    n = len(which)
    zd, zi = (C.c_uint32 * (8 * n))(), (C.c_uint32 * (8 * n))()
    h.hs_coset_recover_factors(zd, zi, (C.c_uint32 * max(len(miss), 1))(*miss), C.c_uint32(len(miss)),
                               (C.c_uint32 * n)(*which), C.c_uint32(n), C.c_int(e), C.c_uint32(parts), roots_raw,
                               (C.c_uint32 * 8)(*X.limbs(pow(7, 1 << e, R))))
    val = lambda a, c: sum(a[8 * c + i] << (32 * i) for i in range(8))
    return [val(zd, c) for c in range(n)], [val(zi, c) for c in range(n)]


def _missing_sets(e):
    m = 8192 >> e
    rnd = random.Random(900 + e)
    return {"random_half": sorted(rnd.sample(range(m), m // 2)),
            "odd_count": sorted(rnd.sample(range(m), m // 2 - 5)),       # no multiple of any parts > 1
            "three": sorted(rnd.sample(range(m), 3)),                    # fewer than parts
            "none": []}


@pytest.mark.parametrize("e", ES)
def test_factors_are_the_two_products(h, roots_raw, e):
    m = 8192 >> e
    for name, missing in _missing_sets(e).items():
        if e >= 3:
            which = list(range(m))
        else:   # the full product is 67 M big-integer multiplications at e = 0: a fixed sample of 64 cosets or more
            rnd = random.Random(e)
            gone = set(missing)
            held = [c for c in range(m) if c not in gone]
            which = sorted(set([0, m - 1, held[len(held) // 2]] + missing[:1] + [rnd.randrange(m) for _ in range(80)]))
            assert len(which) >= 64 or not missing
        want_d, want_i = X.factors(missing, which, e)
        for parts in X.all_parts(e):
            zd, zi = _replay(h, roots_raw, missing, which, e, parts)
            assert zd == want_d, (name, parts)
            assert zi == want_i, (name, parts)
        for i, c in enumerate(which):
            assert (want_d[i] == 0) == (c in missing)
        if not missing:
            assert set(want_d) == {1} and set(want_i) == {1}


@pytest.mark.parametrize("e", ES)
@pytest.mark.parametrize("first", [True, False])
def test_factors_of_the_half_sets_are_the_closed_forms(h, roots_raw, e, first):
    m = 8192 >> e
    missing = list(range(m // 2)) if first else list(range(m // 2, m))
    which = list(range(m))
    zd, zi = _replay(h, roots_raw, missing, which, e, X.parts(1, e))
    for c in which:
        d, s = X.closed_form(first, c, e)
        assert zd[c] == d and zi[c] * s % R == 1
        assert d == (0 if (c < m // 2) == first else (R - 2 if first else 2))
