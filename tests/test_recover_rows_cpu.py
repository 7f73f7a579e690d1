"""ckzg_hip_recover_cells_and_kzg_proofs_rows without a GPU: the symbol is declared and exported, a settings struct
without GPU state gives C_KZG_ERROR (no CPU fallback), the binding checks its arguments, the index maps the product
builds (csrc/coset_recover_plan.hpp at e = 6, through libhost_shim.so) put every cell at (its row, its column) and give equal
set ids exactly to equal sets, and the per-cell factors of csrc/coset_recover_factors.hpp -- the function the kernel
calls, replayed on the host -- are the vanishing polynomial of the missing cells: equal to the two products computed
with Python integers, and equal to Z evaluated from the coefficients that the existing route's recurrence
(vanishing_poly_from_roots, recovery.c:46-75) gives."""
import ctypes as C
import os
import random
import subprocess

import pytest

from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, Kzg, KzgError, KZGSettings
from test_abi_exports import declared_symbols

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NAME = "ckzg_hip_recover_cells_and_kzg_proofs_rows"
W = pow(7, (R - 1) // 8192, R)          # the 8192nd root of unity of the settings (roots_of_unity[1])
W128 = pow(W, 64, R)
SEVEN64 = pow(7, 64, R)
NONE = 0xffffffff


def brp(v, bits):
    return int(format(v, "0%db" % bits)[::-1], 2)


def test_symbol_declared_and_exported():
    assert NAME in declared_symbols()
    assert "    %s;\n" % NAME in open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    assert hasattr(C.CDLL(HIP_SO), NAME)


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    f = getattr(C.CDLL(HIP_SO), NAME)
    f.restype = C.c_int
    s = KZGSettings()
    rc, rp, st = C.create_string_buffer(128 * 2048), C.create_string_buffer(128 * 48), (C.c_uint8 * 1)()
    idx = (C.c_uint64 * 64)(*range(64))
    start = (C.c_uint64 * 2)(0, 64)
    assert f(rc, rp, st, idx, bytes(64 * 2048), start, C.c_uint64(1), C.byref(s)) == 2
    assert f(None, None, None, None, None, None, C.c_uint64(0), C.byref(s)) == 2
    assert rc.raw == bytes(128 * 2048) and rp.raw == bytes(128 * 48)


def test_binding_checks_its_arguments():
    api = Kzg.__new__(Kzg)   # no library: every check below fails before a call is made
    cell = bytes(2048)
    for rows in ([([0], [cell], [cell])],                 # not two lists
                 [([0, 1], [cell])],                      # list lengths
                 [([0], [cell[:-1]])],                    # a short cell
                 [([0], [cell + b"0"])],                  # a long cell
                 [([-1], [cell])],                        # an index that is no uint64
                 [([1 << 64], [cell])],
                 [([0.5], [cell])]):
        with pytest.raises(KzgError):
            api.recover_cells_and_kzg_proofs_rows(rows)
    with pytest.raises(KzgError):
        api.recover_cells_and_kzg_proofs_rows([([0], [cell])], False, False)


# ---- the plan ----

@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    assert hasattr(lib, "hs_recover_rows_plan") and hasattr(lib, "hs_recover_set_factors")
    lib.hs_recover_rows_plan.restype = C.c_long
    lib.hs_recover_set_factors.restype = None
    return lib


def _plan(h, rows, chunk_rows, start=None):
    nr = len(rows)
    if start is None:
        start = [0]
        for r in rows:
            start.append(start[-1] + len(r))
    flat = [c for r in rows for c in r]
    n = max(len(flat), 1)
    valid = (C.c_uint8 * max(nr, 1))()
    per_row = [(C.c_uint32 * max(nr, 1))() for _ in range(3)]
    mask = (C.c_uint32 * (4 * max(nr, 1)))()
    cell_pos, cell_dst = (C.c_uint32 * n)(), (C.c_uint32 * n)()
    cap = nr + 1
    info = (C.c_uint32 * (4 * cap))()
    ret = h.hs_recover_rows_plan(valid, per_row[0], per_row[1], per_row[2], mask, cell_pos, cell_dst, info, C.c_size_t(cap),
                                 (C.c_uint64 * n)(*flat), (C.c_uint64 * len(start))(*start), C.c_uint64(nr),
                                 C.c_size_t(chunk_rows))
    return dict(ret=ret, valid=list(valid)[:nr], chunk=list(per_row[0])[:nr], dev=list(per_row[1])[:nr],
                set=list(per_row[2])[:nr], mask=[tuple(mask[4 * r:4 * r + 4]) for r in range(nr)],
                cell_pos=list(cell_pos), cell_dst=list(cell_dst), info=[tuple(info[4 * c:4 * c + 4]) for c in range(cap)],
                start=start)


def _mask_words(cols):
    m = sum(1 << c for c in cols)
    return tuple((m >> (32 * w)) & 0xffffffff for w in range(4))


def _mixed_rows(seed):
    rnd = random.Random(seed)
    sets = [list(range(0, 128, 2)), list(range(64)), list(range(64, 128)), sorted(rnd.sample(range(128), 64)),
            sorted(rnd.sample(range(128), 70)), sorted(rnd.sample(range(128), 127)), list(range(128))]
    good = [list(sets[i % len(sets)]) for i in range(23)]          # every set three times or more
    bad = [list(range(63)), list(range(128)) + [128], list(range(63)) + [128], list(range(62)) + [70, 69],
           list(range(63)) + [62], [], list(range(127, 63, -1)), [5] * 64]
    rows = [(r, True) for r in good] + [(r, False) for r in bad]
    rnd.shuffle(rows)
    return [r for r, _ in rows], [ok for _, ok in rows]


@pytest.mark.parametrize("chunk_rows", [512, 5, 1])
def test_plan_places_every_cell_and_names_the_sets(h, chunk_rows):
    rows, expect_valid = _mixed_rows(11)
    p = _plan(h, rows, chunk_rows)
    nvalid = sum(expect_valid)
    assert p["ret"] == (nvalid + chunk_rows - 1) // chunk_rows
    assert p["valid"] == [int(v) for v in expect_valid]
    # device rows: caller order, packed, chunk_rows per chunk; none for an invalid row
    seen = 0
    for r, ok in enumerate(expect_valid):
        if not ok:
            assert (p["chunk"][r], p["dev"][r], p["set"][r]) == (NONE, NONE, NONE)
            assert all(p["cell_pos"][i] == NONE and p["cell_dst"][i] == NONE for i in range(p["start"][r], p["start"][r + 1]))
            continue
        assert (p["chunk"][r], p["dev"][r]) == (seen // chunk_rows, seen % chunk_rows)
        seen += 1
        assert p["mask"][r] == _mask_words(rows[r])
        # every cell lands at (its row, its column), and the device input is packed in caller order
        for j, col in enumerate(rows[r]):
            assert p["cell_dst"][p["start"][r] + j] == p["dev"][r] * 128 + col
    for c in range(p["ret"]):
        members = [r for r in range(len(rows)) if p["chunk"][r] == c]
        # set ids agree exactly where masks agree, and count from 0 in order of first appearance
        ids = {}
        for r in members:
            assert ids.setdefault(tuple(rows[r]), p["set"][r]) == p["set"][r]
        assert sorted(ids.values()) == list(range(len(ids)))
        assert [ids[k] for k in ids] == sorted(ids.values())
        pos = [p["cell_pos"][i] for r in members for i in range(p["start"][r], p["start"][r + 1])]
        assert pos == list(range(len(pos)))
        assert p["info"][c] == (len(members), len(pos), len(ids), int(all(len(rows[r]) == 128 for r in members)))


def test_plan_all_full_chunk_and_empty_call(h):
    p = _plan(h, [list(range(128))] * 3, 512)
    assert p["ret"] == 1 and p["info"][0] == (3, 384, 1, 1)
    p = _plan(h, [], 512)
    assert p["ret"] == 0
    p = _plan(h, [list(range(10))], 512)
    assert p["ret"] == 0 and p["valid"] == [0]


def test_plan_rejects_malformed_row_start(h):
    rows = [list(range(64)), list(range(64))]
    assert _plan(h, rows, 512, start=[1, 64, 128])["ret"] == -1       # does not start at 0
    assert _plan(h, rows, 512, start=[0, 128, 64])["ret"] == -1       # decreases
    assert _plan(h, rows, 512, start=[0, 64, 128])["ret"] == 1


# ---- the factors ----

def _limbs(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def _factors(h, cols):
    roots = (C.c_uint32 * (8 * 8193))()
    v = 1
    for i in range(8193):
        roots[8 * i:8 * i + 8] = _limbs(v)
        v = v * W % R
    zd, zi = (C.c_uint32 * (8 * 128))(), (C.c_uint32 * (8 * 128))()
    h.hs_recover_set_factors(zd, zi, (C.c_uint32 * 4)(*_mask_words(cols)), roots, (C.c_uint32 * 8)(*_limbs(SEVEN64)))
    val = lambda a, c: sum(a[8 * c + i] << (32 * i) for i in range(8))
    return [val(zd, c) for c in range(128)], [val(zi, c) for c in range(128)]


def _sets():
    rnd = random.Random(2024)
    return {"even": list(range(0, 128, 2)), "first_64": list(range(64)), "last_64": list(range(64, 128)),
            "random_64": sorted(rnd.sample(range(128), 64)), "random_70": sorted(rnd.sample(range(128), 70)),
            "127_cells": sorted(rnd.sample(range(128), 127)), "all_128": list(range(128))}


@pytest.mark.parametrize("name", list(_sets()))
def test_factors_are_the_two_products(h, name):
    cols = _sets()[name]
    missing = [j for j in range(128) if j not in cols]
    zd, zi = _factors(h, cols)
    for c in range(128):
        x = pow(W128, brp(c, 7), R)
        pd = pc = 1
        for j in missing:
            rj = pow(W128, brp(j, 7), R)
            pd = pd * (x - rj) % R
            pc = pc * (SEVEN64 * x - rj) % R
        assert zd[c] == pd
        assert (pd == 0) == (c in missing)
        assert pc != 0 and zi[c] == pow(pc, R - 2, R)


def test_factors_are_the_vanishing_polynomial_of_the_existing_route(h):
    """Z as RecoverSameCells::prepare builds it: the recurrence of vanishing_poly_from_roots over the roots
    w^(64 brp7(j)) of the missing cells j, its coefficients spread 64 apart, evaluated at w^brp13(p) (the domain in
    the order in which the data is held) and at 7 w^brp13(p) (the coset)."""
    cols = _sets()["random_70"]
    roots = [pow(W, brp(j, 7) * 64, R) for j in range(128) if j not in cols]
    n = len(roots)
    poly = [0] * (n + 1)
    poly[0] = -roots[0] % R
    for i in range(1, n):
        nr = -roots[i] % R
        poly[i] = (nr + poly[i - 1]) % R
        for j in range(i - 1, 0, -1):
            poly[j] = (poly[j] * nr + poly[j - 1]) % R
        poly[0] = poly[0] * nr % R
    poly[n] = 1

    def z(x):
        y, acc = pow(x, 64, R), 0
        for coef in reversed(poly):
            acc = (acc * y + coef) % R
        return acc

    zd, zi = _factors(h, cols)
    rnd = random.Random(7)
    for p in [0, 63, 64, 8191] + [rnd.randrange(8192) for _ in range(200)]:
        x = pow(W, brp(p, 13), R)
        assert zd[p // 64] == z(x)
        assert zi[p // 64] == pow(z(7 * x % R), R - 2, R)
