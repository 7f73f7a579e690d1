"""ckzg_hip_verify_cell_kzg_proof_batch_locate without a GPU: the symbol, the chunk's two-level challenge digest
(csrc/locate_plan.hpp: every byte of every item must reach r -- a verdict cannot show that, so this does), and the whole
second half in host arithmetic (libhost_shim.so: hs_locate_cells_host -- per-cell interpolation by the definition of the
inverse transform, P1, the r^i scaling, prefix sums, the range predicate with the real pairing against [s^64]_2) over
every well-formed verify_cell_kzg_proof_batch consensus vector, flattened into single cells.  Expected verdicts: the CPU
oracle's verify_cell_kzg_proof_batch on each item alone."""
import ctypes as C
import os
import subprocess

import pytest

import cell_locate_items as CL
import g1_points as GP
from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, KZGSettings
from test_abi_exports import declared_symbols

NAME = "ckzg_hip_verify_cell_kzg_proof_batch_locate"


@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    assert hasattr(lib, "hs_locate_cell_digest") and hasattr(lib, "hs_locate_cells_host")
    lib.hs_locate_cell_digest.restype = None
    lib.hs_locate_cells_host.restype = C.c_int
    return lib


def test_symbol_declared_and_exported():
    exports = open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    assert NAME in declared_symbols()
    assert "    %s;\n" % NAME in exports
    assert hasattr(C.CDLL(HIP_SO), NAME)
    src = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    assert "#define CKZG_HIP_CELL_LOCATE_CHUNK_CELLS 16384\n" in src


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    f = getattr(C.CDLL(HIP_SO), NAME)
    f.restype = C.c_int
    s = KZGSettings()
    ok, st, stats = (C.c_bool * 2)(), (C.c_uint8 * 2)(), (C.c_uint64 * 3)()
    assert f(ok, st, stats, bytes(96), (C.c_uint64 * 2)(0, 1), bytes(2 * 2048), bytes(96), C.c_uint64(2), C.byref(s)) == 2


# ---- the digest ----

def _digest(h, items):
    n = len(items)
    out = C.create_string_buffer(32)
    j = lambda k: b"".join(t[k] for t in items)
    h.hs_locate_cell_digest(out, j(0), (C.c_uint64 * max(n, 1))(*[t[1] for t in items]), j(2), j(3), C.c_uint64(n))
    return out.raw


def _made_items(n):
    """n items of distinct bytes (no curve points: the digest is over bytes)"""
    import hashlib
    x = lambda tag, i, size: hashlib.shake_128(b"%s/%d" % (tag, i)).digest(size)
    return [(x(b"c", i, 48), (i * 37) % 128, x(b"cell", i, 2048), x(b"p", i, 48)) for i in range(n)]


@pytest.mark.parametrize("k", [1, 2, 5, 257])
def test_digest_is_the_two_level_hash(h, k):
    items = _made_items(k)
    want = CL.digest(items)
    assert _digest(h, items) == want
    # one bit anywhere changes it: a commitment, an index, the first and the last field element of a cell, a proof, the last item
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]
    seen = {want}
    mid = k // 2
    for what, at in (("commitment", 47), ("index", None), ("cell", 0), ("cell", 31), ("cell", 2047), ("cell", 2048 - 32), ("proof", 0),
                     ("last", None)):
        it = [list(t) for t in items]
        if what == "commitment":
            it[mid][0] = flip(it[mid][0], at)
        elif what == "index":
            it[mid][1] ^= 1
        elif what == "cell":
            it[mid][2] = flip(it[mid][2], at)
        elif what == "proof":
            it[mid][3] = flip(it[mid][3], at)
        else:
            it[k - 1][3] = flip(it[k - 1][3], 47)
        got = _digest(h, it)
        assert got == CL.digest(it) and got not in seen, what
        seen.add(got)
    # ... and so does the order of the items, and their number
    if k > 1:
        assert _digest(h, items[::-1]) == CL.digest(items[::-1]) not in seen
        assert _digest(h, items[:-1]) == CL.digest(items[:-1]) not in seen


# ---- the second half on the host, with the real pairing ----

def _g2(h, b96):
    aff = C.create_string_buffer(192)
    assert h.hs_g2_uncompress(aff, b96) == 0
    gen = C.create_string_buffer(288)
    h.hs_g2_generator(gen)
    return aff.raw + gen.raw[192:]


def _cells_host(h, items, max_checks=-1):
    n = len(items)
    ok, st, stats, r32 = (C.c_uint8 * max(n, 1))(), (C.c_uint8 * max(n, 1))(), (C.c_uint64 * 2)(), C.create_string_buffer(32)
    j = lambda k: b"".join(t[k] for t in items)
    assert h.hs_locate_cells_host(ok, st, stats, r32, j(0), (C.c_uint64 * max(n, 1))(*[t[1] for t in items]), j(2), j(3), C.c_uint64(n),
                                  CL.setup_mono64(), _g2(h, CL.setup_s64_g2()), C.c_int64(max_checks)) == 0
    return [bool(v) for v in ok[:n]], list(st[:n]), stats[0], r32.raw


@pytest.fixture(scope="module")
def items(oracle):
    """every cell of every well-formed vector, then built items so that each kind of outcome is there: a cell with one
    bit flipped, an index of 128, a commitment and a proof outside G1"""
    spec = CL.spec_items()
    assert len(spec) == 925
    good = next(t for t in spec if t[4] is True)
    assert GP.classify(CL.NOT_G1) == GP.NOT_IN_G1
    built = [(good[0], good[1], CL.flip_low_bit(good[2], 17), good[3], None, "built: bit flipped"),
             (good[0], 128, good[2], good[3], None, "built: index 128"),
             (CL.NOT_G1, good[1], good[2], good[3], None, "built: commitment outside G1"),
             (good[0], good[1], good[2], CL.NOT_G1, None, "built: proof outside G1"),
             (good[0], good[1], CL.non_canonical(good[2], 63), good[3], None, "built: non-canonical element")]
    all_items = spec[:400] + built + spec[400:]
    return all_items, [CL.verdict(oracle, t) for t in all_items]


def test_all_spec_vectors_on_the_host(h, items):
    all_items, want = items
    assert set(want) == {(True, 0), (False, 0), (False, CL.BADARGS)}
    ok, st, checks, r32 = _cells_host(h, all_items)
    for i, (t, w) in enumerate(zip(all_items, want)):
        assert (ok[i], st[i]) == w, (i, t[5], t[1], ok[i], st[i], w)
        if t[4] is True:   # every item of a vector that verifies comes out true
            assert ok[i] is True and st[i] == 0, (i, t[5])
    nfalse = want.count((False, 0))
    assert nfalse >= 1 and 1 < checks <= 1 + 2 * nfalse * CL.ceil_log2(len(all_items))
    assert r32 == CL.digest(all_items)


def test_true_items_alone_cost_one_check(h, items):
    all_items, want = items
    true_items = [t for t, w in zip(all_items, want) if w == (True, 0)][:200]
    invalid = [t for t, w in zip(all_items, want) if w == (False, CL.BADARGS)]
    assert len(true_items) == 200 and len(invalid) >= 4
    ok, st, checks, _ = _cells_host(h, true_items)
    assert ok == [True] * 200 and st == [0] * 200 and checks == 1
    # invalid items in a good batch are settled from their flags: still one check
    mixed = invalid[:1] + true_items[:5] + invalid[1:3] + true_items[5:] + invalid[3:]
    ok, st, checks, _ = _cells_host(h, mixed)
    assert checks == 1
    assert ok == [t in true_items for t in mixed] and st == [0 if t in true_items else 1 for t in mixed]
    # no valid item: no check at all
    ok, st, checks, _ = _cells_host(h, invalid)
    assert checks == 0 and ok == [False] * len(invalid) and st == [1] * len(invalid)
