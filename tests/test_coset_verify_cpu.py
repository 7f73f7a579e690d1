"""ckzg_hip_verify_coset_kzg_proof_batch without a GPU: the index maps and launch decisions of
csrc/coset_verify_plan.hpp for every coset size, through libhost_shim.so, against the model
(tests/coset_verify_expect.py); the batch challenge against hashlib at every size and, at e = 6, against the exported
compute_verify_cell_kzg_proof_batch_challenge on the same bytes; the symbol is declared, exported and bound; bad
arguments are rejected before anything looks at the device, and settings without GPU state give C_KZG_ERROR."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess

import pytest

import coset_verify_expect as V
import domain_expect as D
from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, KZGSettings
from test_abi_exports import declared_symbols

NEW = "ckzg_hip_verify_coset_kzg_proof_batch"
HDR = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
R = D.R
U32, U64 = C.c_uint32, C.c_uint64


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    assert hasattr(lib, "hs_coset_verify_brp")
    for n in ("cosets", "brp", "shift_root", "unshift_root", "slot", "twiddle_root", "agg_parts"):
        getattr(lib, "hs_coset_verify_" + n).restype = U32
    return lib


def _constants(shim):
    what = (U64 * 6)()
    shim.hs_coset_verify_constants(what)
    return dict(zip(("per_lane", "max_parts", "hash_on_pool_from", "min_shard", "agg_slots", "interp_threads"), what))


# ---- csrc/coset_verify_plan.hpp ----

@pytest.mark.parametrize("e", range(7))
def test_index_maps_match_the_model_for_every_coset(shim, e):
    l, m = 1 << e, 8192 >> e
    assert shim.hs_coset_verify_cosets(e) == m == V.cosets(e)
    w = D.root_of_unity(8192)
    roots = [1] * 8192
    for i in range(1, 8192):
        roots[i] = roots[i - 1] * w % R
    seen = set()
    for c in range(m):
        b = shim.hs_coset_verify_brp(U32(c), e)
        assert b == V.coset_brp(c, e)
        seen.add(b)
        sh = shim.hs_coset_verify_shift_root(U32(c), e)
        assert sh == V.shift_root(c, e) and roots[sh] == pow(roots[b], l, R)
        for k in sorted({0, 1, l // 2, l - 1}):
            un = shim.hs_coset_verify_unshift_root(U32(c), e, U32(k))
            assert un == V.unshift_root(c, e, k) and roots[un] * pow(roots[b], k, R) % R == 1
        for j in sorted({0, l - 1}):
            assert shim.hs_coset_verify_slot(U32(c), e, U32(j)) == V.slot(c, e, j) == c * l + j
    assert seen == set(range(m))
    for s in range(1, e + 1):
        for pos in range(l):
            t = shim.hs_coset_verify_twiddle_root(U32(pos), s)
            assert t == V.twiddle_root(pos, s)
            assert roots[t] == pow(w, -(pos % (1 << (s - 1))) * (8192 >> s), R)


def test_points_of_a_coset_are_the_interface_order(shim):
    """x_c w_l^brp_e(j) from the maps = brp_roots_of_unity[c l + j] of the 8192-point domain"""
    w = D.root_of_unity(8192)
    for e in range(7):
        l = 1 << e
        for c in (0, 1, (8192 >> e) - 1):
            x = pow(w, shim.hs_coset_verify_brp(U32(c), e), R)
            for j in range(l):
                assert x * pow(w, (8192 // l) * D.brp(j, e), R) % R == pow(w, D.brp(c * l + j, 13), R)


def test_aggregate_split(shim):
    k = _constants(shim)
    assert k["agg_slots"] == 64 and 8192 % k["interp_threads"] == 0 and k["interp_threads"] % 64 == 0
    for e in range(7):
        m = 8192 >> e
        edge = m * k["per_lane"]
        for items in (0, 1, edge - 1, edge, edge + 1, 2 * edge, 2 * edge + 1, 8 * edge + 1, 1 << 23):
            got = shim.hs_coset_verify_agg_parts(U64(items), e)
            assert got == V.agg_parts(items, e, k["per_lane"], k["max_parts"])
            assert got & (got - 1) == 0 and 1 <= got <= k["max_parts"]
            assert got * k["agg_slots"] <= 1024 and got * k["agg_slots"] * 32 <= 65536     # threads, LDS bytes
        assert shim.hs_coset_verify_agg_parts(U64(edge), e) == 1
        assert shim.hs_coset_verify_agg_parts(U64(edge + 1), e) == 2


# ---- the challenge ----

def _batch(e, n, rnd):
    cms = [bytes([0x80 + (i % 3)]) + rnd.randbytes(47) for i in range(3)]
    cm = [cms[rnd.randrange(3)] for _ in range(n)]
    idx = [rnd.randrange(8192 >> e) for _ in range(n)]
    ev = [rnd.randbytes(32 << e) for _ in range(n)]
    pf = [rnd.randbytes(48) for _ in range(n)]
    return cm, idx, ev, pf


def _shim_digest(shim, cm, idx, ev, pf, e):
    uniq = []
    for c in cm:
        if c not in uniq:
            uniq.append(c)
    n = len(ev)
    out = C.create_string_buffer(32)
    shim.hs_coset_verify_digest(out, b"".join(uniq), U64(len(uniq)), (U64 * max(n, 1))(*[uniq.index(c) for c in cm]),
                                (U64 * max(n, 1))(*idx), b"".join(ev), b"".join(pf), U64(n), e)
    return out.raw, uniq


@pytest.mark.parametrize("e", range(7))
def test_challenge_is_the_models(shim, e):
    rnd = random.Random(77 + e)
    for n in (1, 2, 5):
        cm, idx, ev, pf = _batch(e, n, rnd)
        digest, _ = _shim_digest(shim, cm, idx, ev, pf, e)
        assert digest == hashlib.sha256(V.transcript(cm, idx, ev, pf, e)).digest()
        assert int.from_bytes(digest, "big") % R == V.challenge(cm, idx, ev, pf, e)


def test_challenge_at_64_is_the_cell_challenge(shim):
    rnd = random.Random(6)
    cm, idx, ev, pf = _batch(6, 4, rnd)
    digest, uniq = _shim_digest(shim, cm, idx, ev, pf, 6)
    lib = C.CDLL(HIP_SO)
    f = lib.compute_verify_cell_kzg_proof_batch_challenge
    f.restype = C.c_int
    out = C.create_string_buffer(32)   # an fr_t: Montgomery form; compared through bytes_from_bls_field
    assert f(out, b"".join(uniq), U64(len(uniq)), (U64 * 4)(*[uniq.index(c) for c in cm]), (U64 * 4)(*idx), b"".join(ev),
             b"".join(pf), U64(4)) == 0
    be = C.create_string_buffer(32)
    lib.bytes_from_bls_field(be, out)
    assert int.from_bytes(be.raw, "big") == int.from_bytes(digest, "big") % R


# ---- the symbol ----

def test_symbol_declared_exported_and_bound():
    exports = open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    binding = open(os.path.join(ROOT, "c-kzg-4844_amd", "ckzg.py")).read()
    assert NEW in declared_symbols()
    assert "    %s;\n" % NEW in exports
    assert hasattr(C.CDLL(HIP_SO), NEW)
    assert '"%s"' % NEW in binding
    assert "def verify_coset_kzg_proof_batch(self, commitments, coset_indices, evals, proofs, log2_coset)" in binding
    assert "NO verifier" not in HDR and "NO verifier" not in open(os.path.join(ROOT, "README.md")).read()


def _fn():
    f = getattr(C.CDLL(HIP_SO), NEW)
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    return f


def test_bad_arguments_are_rejected_before_any_gpu_work():
    """(a zeroed settings struct: a check that came after the first look at the device would answer C_KZG_ERROR)"""
    s, f = KZGSettings(), _fn()
    cm, ev, pf = C.create_string_buffer(48), C.create_string_buffer(2048), C.create_string_buffer(48)
    idx = (U64 * 1)(0)
    for e in (7, 8, 13, 64, 2 ** 32 - 1):
        ok = C.c_bool(True)
        assert f(C.byref(ok), cm, idx, ev, pf, 1, e, C.byref(s)) == 1 and not ok.value
        ok = C.c_bool(True)
        assert f(C.byref(ok), None, None, None, None, 0, e, C.byref(s)) == 1 and not ok.value
    for e in range(7):
        for args in ((None, idx, ev, pf), (cm, None, ev, pf), (cm, idx, None, pf), (cm, idx, ev, None)):
            ok = C.c_bool(True)
            assert f(C.byref(ok), *args, 1, e, C.byref(s)) == 1 and not ok.value
        for c in (8192 >> e, 8192, 2 ** 64 - 1):
            ok = C.c_bool(True)
            assert f(C.byref(ok), cm, (U64 * 1)(c), ev, pf, 1, e, C.byref(s)) == 1 and not ok.value
    assert f(None, cm, idx, ev, pf, 1, 0, C.byref(s)) == 1


def test_nothing_to_do_is_true_and_zeroed_settings_give_error():
    s, f = KZGSettings(), _fn()
    cm, ev, pf = C.create_string_buffer(48), C.create_string_buffer(2048), C.create_string_buffer(48)
    for e in range(7):
        ok = C.c_bool(False)
        assert f(C.byref(ok), None, None, None, None, 0, e, C.byref(s)) == 0 and ok.value
        ok = C.c_bool(True)
        assert f(C.byref(ok), cm, (U64 * 1)((8192 >> e) - 1), ev, pf, 1, e, C.byref(s)) == 2 and not ok.value   # no CPU fallback
