"""ckzg_hip_verify_coset_kzg_proof_batch_locate without a GPU: the symbol and its argument checks, the chunk's two-level
challenge digest (csrc/locate_plan.hpp: every byte of every item, and l, must reach r), the launch plan
(csrc/coset_locate_plan.hpp against its restatement in tests/coset_locate_expect.py), and the whole second half in host
arithmetic at every coset size (libhost_shim.so: hs_locate_cosets_host -- per-item interpolation by the definition of
the inverse transform, P1, the r^i scaling, prefix sums, the range predicate with the real pairing against [s^l]_2).

The items are made on the CPU: the 64 openings of the oracle's compute_kzg_proof at the points of one cell, folded
upwards with proof_e[c] = [1 / (2a)](proof_{e-1}[2c] - proof_{e-1}[2c+1]) in the oracle's group arithmetic; the top of
the ladder must be the oracle's cell proof.  Expected verdicts: the oracle's verify_kzg_proof at e = 0, its
verify_cell_kzg_proof_batch on the item alone at e = 6, the check by definition on the setup file's points between."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

import cell_locate_items as CL
import coset_locate_expect as X
import g1_points as GP
from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, KZGSettings, KzgError, TRUSTED_SETUP
from test_abi_exports import declared_symbols
from test_gpu_coset_openings import EXT, ZS, _compress, _jac
from test_gpu_coset_verify import Setup, _bump
from test_gpu_locate import G1
from test_gpu_point_openings import _blob

NAME = "ckzg_hip_verify_coset_kzg_proof_batch_locate"
R = X.R
ES = list(range(7))
CELL = 77   # the cell whose 64 points are opened


@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    assert hasattr(lib, "hs_locate_coset_digest") and hasattr(lib, "hs_locate_cosets_host")
    lib.hs_locate_coset_digest.restype = None
    lib.hs_locate_cosets_host.restype = C.c_int
    lib.hs_coset_locate_chunk_items.restype = C.c_uint64
    lib.hs_coset_locate_sum_lpv.restype = C.c_int
    return lib


def test_symbol_declared_and_exported():
    exports = open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    assert NAME in declared_symbols()
    assert "    %s;\n" % NAME in exports
    assert hasattr(C.CDLL(HIP_SO), NAME)
    src = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    assert "#define CKZG_HIP_COSET_LOCATE_CHUNK_SLOTS 1048576\n" in src


def _raw_call(e, s, ok, n=2):
    f = getattr(C.CDLL(HIP_SO), NAME)
    f.restype = C.c_int
    st, stats = (C.c_uint8 * n)(), (C.c_uint64 * 3)()
    return f(ok, st, stats, bytes(48 * n), (C.c_uint64 * n)(0, 1), bytes(n * (32 << min(e, 6))), bytes(48 * n), C.c_uint64(n),
             C.c_uint32(e), C.byref(s))


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    for e in ES:
        assert _raw_call(e, KZGSettings(), (C.c_bool * 2)()) == 2


def test_coset_size_out_of_range_is_refused_before_anything_is_written():
    ok = (C.c_bool * 2)(True, True)
    assert _raw_call(7, KZGSettings(), ok) == 1
    assert list(ok) == [True, True]
    assert _raw_call(0xFFFFFFFF, KZGSettings(), ok) == 1 and list(ok) == [True, True]


# ---- the plan ----

def test_plan_is_its_restatement(h):
    what = (C.c_uint64 * 15)()
    h.hs_coset_locate_constants(what)
    assert list(what[:7]) == X.WAVE_BELOW and list(what[7:14]) == X.LPV and what[14] == X.MIN_SHARD
    for e in ES:
        assert h.hs_coset_locate_chunk_items(e) == X.chunk_items(e)
        for at in X.switch_points(e):
            for n in (1, at - 1, at, at + 1, X.chunk_items(e)):
                assert h.hs_coset_locate_sum_lpv(e, C.c_uint64(n)) == X.sum_lpv(e, n), (e, n)
        assert X.sum_lpv(e, X.switch_points(e)[0] - 1) == 64 and X.sum_lpv(e, X.switch_points(e)[0]) in (4, 8, 16)
    assert [X.chunk_items(e) for e in ES] == [65536] * 5 + [32768, 16384]


# ---- the digest ----

def _digest(h, items, e):
    n = len(items)
    out = C.create_string_buffer(32)
    j = lambda k: b"".join(t[k] for t in items)
    h.hs_locate_coset_digest(out, j(0), (C.c_uint64 * max(n, 1))(*[t[1] for t in items]), j(2), j(3), C.c_uint64(n), C.c_int(e))
    return out.raw


def _made_items(n, e):
    """n items of distinct bytes (no curve points: the digest is over bytes)"""
    x = lambda tag, i, size: hashlib.shake_128(b"%s/%d/%d" % (tag, e, i)).digest(size)
    return [(x(b"c", i, 48), (i * 37) % (8192 >> e), x(b"v", i, 32 << e), x(b"p", i, 48)) for i in range(n)]


@pytest.mark.parametrize("k", [1, 2, 5, 257])
@pytest.mark.parametrize("e", ES)
def test_digest_is_the_two_level_hash(h, e, k):
    items = _made_items(k, e)
    want = X.digest(items, e)
    assert _digest(h, items, e) == want
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]
    seen = {want}
    mid, nv = k // 2, 32 << e
    cases = [("commitment", 47), ("index", None)] + [("value", at) for at in sorted({0, 31, nv - 32, nv - 1})] + [("proof", 0), ("last", None)]
    for what, at in cases:
        it = [list(t) for t in items]
        if what == "commitment":
            it[mid][0] = flip(it[mid][0], at)
        elif what == "index":
            it[mid][1] ^= 1
        elif what == "value":
            it[mid][2] = flip(it[mid][2], at)
        elif what == "proof":
            it[mid][3] = flip(it[mid][3], at)
        else:
            it[k - 1][3] = flip(it[k - 1][3], 47)
        got = _digest(h, it, e)
        assert got == X.digest(it, e) and got not in seen, (what, at)
        seen.add(got)
    # l is hashed, in the leaves and in the root: the same bytes under another l give another digest
    for other in (2 << e, (1 << e) >> 1, (1 << e) ^ (1 << 40)):
        assert X.digest(items, e, l_field=other) not in seen
    if e < 6:   # ... and the same buffers read at the next size
        assert _digest(h, [(t[0], t[1], t[2] + t[2], t[3]) for t in items], e + 1) not in seen
    if k > 1:
        assert _digest(h, items[::-1], e) == X.digest(items[::-1], e) not in seen
        assert _digest(h, items[:-1], e) == X.digest(items[:-1], e) not in seen


# ---- the second half on the host, with the real pairing ----

def _g2(h, b96):
    aff = C.create_string_buffer(192)
    assert h.hs_g2_uncompress(aff, b96) == 0
    gen = C.create_string_buffer(288)
    h.hs_g2_generator(gen)
    return aff.raw + gen.raw[192:]


def _setup_g2(l):
    return bytes.fromhex(CL.setup_lines()[2 + 4096 + l])


def _cosets_host(h, items, e, max_checks=-1):
    n = len(items)
    ok, st, stats, r32 = (C.c_uint8 * max(n, 1))(), (C.c_uint8 * max(n, 1))(), (C.c_uint64 * 2)(), C.create_string_buffer(32)
    j = lambda k: b"".join(t[k] for t in items)
    assert h.hs_locate_cosets_host(ok, st, stats, r32, j(0), (C.c_uint64 * max(n, 1))(*[t[1] for t in items]), j(2), j(3), C.c_uint64(n),
                                   C.c_int(e), CL.setup_mono64(), _g2(h, _setup_g2(1 << e)), C.c_int64(max_checks)) == 0
    return [bool(v) for v in ok[:n]], list(st[:n]), stats[0], r32.raw


class Ladder:
    """per blob, the openings of one cell's 64 points at every coset size: level[e][i] is the item of coset
    (CELL << (6 - e)) + i, made from the oracle's size-one openings alone"""

    def __init__(self, oracle, g1, seeds):
        self.items = {e: [] for e in ES}
        self.commit = []
        for seed in seeds:
            blob = _blob(seed)
            cm = oracle.blob_to_kzg_commitment(blob)
            self.commit.append(cm)
            opened = [oracle.compute_kzg_proof(blob, EXT[64 * CELL + j]) for j in range(64)]
            ys = [y for _, y in opened]
            level = [_jac(g1, p) for p, _ in opened]
            for e in ES:
                if e:
                    nxt = []
                    for i in range(len(level) // 2):
                        a = pow(ZS[((CELL << (6 - e)) + i) << e], 1 << (e - 1), R)
                        nxt.append(g1.mul(g1.add(level[2 * i], g1.neg(level[2 * i + 1])), pow(2 * a, -1, R)))
                    level = nxt
                l = 1 << e
                self.items[e].append([(cm, (CELL << (6 - e)) + i, b"".join(ys[i * l:(i + 1) * l]), _compress(g1, level[i]))
                                      for i in range(64 >> e)])
            # the anchor: the top of the ladder is the oracle's cell proof, and the 64 values are its cell
            cells, proofs = oracle.compute_cells_and_kzg_proofs(blob)
            assert self.items[6][-1][0][3] == proofs[CELL] and self.items[6][-1][0][2] == cells[CELL]


@pytest.fixture(scope="module")
def g1():
    return G1()


@pytest.fixture(scope="module")
def ladder(oracle, g1):
    return Ladder(oracle, g1, (0xC10C, 0xC10D))


@pytest.fixture(scope="module")
def setup(g1):
    return Setup(g1)


def _expected(oracle, setup, item, e):
    """(ok, status) of the item alone, from outside the library"""
    cm, c, ev, pf = item
    invalid = c >= 8192 >> e or any(int.from_bytes(ev[k:k + 32], "big") >= R for k in range(0, len(ev), 32)) or \
        GP.classify(cm) != GP.VALID or GP.classify(pf) != GP.VALID
    if e == 0:
        if invalid:
            return (False, X.BADARGS)
        return (oracle.verify_kzg_proof(cm, EXT[c], ev, pf), 0)
    if e == 6:
        try:
            got = (oracle.verify_cell_kzg_proof_batch([cm], [c], [ev], [pf]), 0)
        except KzgError:
            got = (False, X.BADARGS)
        assert (got[1] == X.BADARGS) == invalid
        return got
    return (False, X.BADARGS) if invalid else (setup.holds(item, e), 0)


def _batch(ladder, e):
    """true items of both blobs with, between them, one bumped value, one foreign proof, one index off by one and one
    invalid item of each kind"""
    a, b = ladder.items[e]
    m = 8192 >> e
    t0, t1 = a[0], b[0]
    other = a[1] if len(a) > 1 else b[0]
    l = 1 << e
    r32 = R.to_bytes(32, "big")
    batch = [t0, t1, _bump(t0, l - 1), a[-1], (t0[0], t0[1], t0[2], other[3]), b[-1], (t0[0], (t0[1] + 1) % m, t0[2], t0[3]),
             (t0[0], m, t0[2], t0[3]), t1, (t1[0], t1[1], t1[2][:32 * (l - 1)] + r32, t1[3]), (CL.NOT_G1, t0[1], t0[2], t0[3]),
             (t0[0], t0[1], t0[2], CL.NOT_G1), t0, _bump(t1, 0), t1]
    return batch


@pytest.mark.parametrize("e", ES)
def test_every_size_on_the_host(h, oracle, setup, ladder, e):
    assert GP.classify(CL.NOT_G1) == GP.NOT_IN_G1
    batch = _batch(ladder, e)
    want = [_expected(oracle, setup, t, e) for t in batch]
    assert want == [(True, 0), (True, 0), (False, 0), (True, 0), (False, 0), (True, 0), (False, 0), (False, 1), (True, 0), (False, 1),
                    (False, 1), (False, 1), (True, 0), (False, 0), (True, 0)]
    ok, st, checks, r32 = _cosets_host(h, batch, e)
    assert list(zip(ok, st)) == want
    nfalse = want.count((False, 0))
    assert 1 < checks <= X.checks_bound(nfalse, len(batch))
    assert r32 == X.digest(batch, e)
    # the true items alone, with the invalid ones among them: one check; nothing valid: none
    true_items = [t for t, w in zip(batch, want) if w == (True, 0)]
    invalid = [t for t, w in zip(batch, want) if w[1] == 1]
    mixed = invalid[:1] + true_items[:3] + invalid[1:3] + true_items[3:] + invalid[3:]
    ok, st, checks, _ = _cosets_host(h, mixed, e)
    assert checks == 1 and ok == [t in true_items for t in mixed] and st == [0 if t in true_items else 1 for t in mixed]
    ok, st, checks, _ = _cosets_host(h, invalid, e)
    assert checks == 0 and ok == [False] * len(invalid) and st == [1] * len(invalid)
    # every item of the ladder's level is true
    level = ladder.items[e][0] + ladder.items[e][1]
    ok, st, checks, _ = _cosets_host(h, level[:16], e)
    assert all(ok) and not any(st) and checks == 1
