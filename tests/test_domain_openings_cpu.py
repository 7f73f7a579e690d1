"""ckzg_hip_g1_fft and ckzg_hip_compute_domain_kzg_proofs_batch(_device) without a GPU: the layout of the single-point
FK20 (tests/domain_expect.py) against the definition of the quotient for N = 2 .. 64; the three symbols are declared and
exported; a settings struct without GPU state gives C_KZG_ERROR (no CPU fallback); NULL and bad-length arguments give
C_KZG_BADARGS before anything else; the index maps, the form picker and the chunk split of csrc/g1_fft_plan.hpp at their
edges, through libhost_shim.so."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import domain_expect as D
from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, KZGSettings
from test_abi_exports import declared_symbols

NEW = ("ckzg_hip_g1_fft", "ckzg_hip_compute_domain_kzg_proofs_batch", "ckzg_hip_compute_domain_kzg_proofs_batch_device")
R = D.R


# ---- the model ----

@pytest.mark.parametrize("N", [2, 4, 8, 16, 32, 64])
def test_layout_against_the_definition(N):
    rnd = random.Random(N)
    s = rnd.randrange(2, R)
    polys = [[rnd.randrange(R) for _ in range(N)],
             [0] * N, [5] + [0] * (N - 1),                 # zero and a constant: every opening is the identity
             [3, 7] + [0] * (N - 2),                       # a + bX: every opening is [b]
             [0] * (N - 1) + [1],                          # X^(N-1): the only term in circulant slot 0
             [0] * (N - 2) + [1, 0] if N > 2 else [0, 1],  # X^(N-2): the only term in the last slot
             [0, 1] + [0] * (N - 2)]                       # X: the only term in slot N+2 (N > 2)
    for c in polys:
        h, pi = D.openings_by_layout(c, s, N)
        assert h == D.h_by_definition(c, s, N)
        assert h[N - 1] == 0
        assert pi == D.openings_by_definition(c, s, N)
    assert D.openings_by_layout(polys[1], s, N)[1] == [0] * N and D.openings_by_layout(polys[2], s, N)[1] == [0] * N
    assert D.openings_by_layout(polys[3], s, N)[1] == [7] * N


def test_circulant_slots_of_the_three_monomials():
    N = 16
    assert D.circulant([0] * (N - 1) + [1]) == [1] + [0] * (2 * N - 1)
    assert D.circulant([0] * (N - 2) + [1, 0]) == [0] * (2 * N - 1) + [1]
    v = D.circulant([0, 1] + [0] * (N - 2))
    assert v[N + 2] == 1 and sum(v) == 1
    assert D.circulant([1] + [0] * (N - 1)) == [0] * (2 * N)   # c_0 is in no quotient


def test_opening_is_the_quotient_at_a_domain_point():
    """independent of both forms above: pi(x) (s - x) = p(s) - p(x) for x = w^k"""
    N, rnd = 32, random.Random(7)
    s, c = rnd.randrange(2, R), [rnd.randrange(R) for _ in range(32)]
    pi = D.openings_by_layout(c, s, N)[1]
    w = D.root_of_unity(N)
    ev = lambda x: sum(a * pow(x, i, R) for i, a in enumerate(c)) % R
    for k in range(N):
        x = pow(w, k, R)
        assert pi[k] * (s - x) % R == (ev(s) - ev(x)) % R


# ---- the symbols ----

def test_symbols_declared_and_exported():
    names = declared_symbols()
    exports = open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    lib = C.CDLL(HIP_SO)
    for n in NEW:
        assert n in names, n
        assert "    %s;\n" % n in exports, n
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    assert re.search(r"#define CKZG_HIP_DOMAIN_CHUNK_BLOBS (\d+)", hdr)


def _fns():
    lib = C.CDLL(HIP_SO)
    f, g, h = (getattr(lib, n) for n in NEW)
    for x in (f, g, h):
        x.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
    g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    return f, g, h


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    f, g, h = _fns()
    s = KZGSettings()
    out, pts = C.create_string_buffer(2 * 144), C.create_string_buffer(2 * 144)
    assert f(out, pts, 2, 1, 0, C.byref(s)) == 2
    assert f(out, pts, 1, 2, 1, C.byref(s)) == 2
    assert f(None, None, 0, 0, 0, C.byref(s)) == 2
    proofs, st, blob = C.create_string_buffer(4096 * 48), (C.c_uint8 * 1)(), C.create_string_buffer(131072)
    assert g(proofs, st, blob, 1, C.byref(s)) == 2
    assert g(None, None, None, 0, C.byref(s)) == 2
    assert h(proofs, st, blob, 1, C.byref(s)) == 2
    assert h(None, None, None, 0, C.byref(s)) == 2
    assert out.raw == bytes(2 * 144) and proofs.raw == bytes(4096 * 48)


def test_bad_arguments_are_rejected_before_any_gpu_work():
    """(a zeroed settings struct: a check that came after the first look at the device would answer C_KZG_ERROR)"""
    f, g, h = _fns()
    s = KZGSettings()
    out, pts = C.create_string_buffer(8 * 144), C.create_string_buffer(8 * 144)
    for n in (3, 6, 12, 8191, 8193, 16384, 2 ** 40, 2 ** 63):
        assert f(out, pts, n, 1, 0, C.byref(s)) == 1, n
        assert f(out, pts, n, 0, 0, C.byref(s)) == 1, n
    assert f(None, pts, 8, 1, 0, C.byref(s)) == 1
    assert f(out, None, 8, 1, 1, C.byref(s)) == 1
    assert f(out, pts, 8192, 2 ** 60, 0, C.byref(s)) == 1   # more points than any device holds
    proofs, blob = C.create_string_buffer(48), C.create_string_buffer(32)
    for fn in (g, h):
        assert fn(None, None, blob, 1, C.byref(s)) == 1
        assert fn(proofs, None, None, 1, C.byref(s)) == 1
    assert out.raw == bytes(8 * 144)


# ---- csrc/g1_fft_plan.hpp ----

@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    assert hasattr(lib, "hs_g1_fft_form")
    for n in ("hs_g1_fft_quad_max_default", "hs_domain_chunk_count", "hs_domain_chunk_size"):
        getattr(lib, n).restype = C.c_uint64
    lib.hs_g1_fft_ladders.restype = C.c_uint32
    return lib


def test_lengths(shim):
    for l in range(14):
        assert shim.hs_g1_fft_log2(C.c_uint64(1 << l)) == l
    for n in (0, 3, 6, 8191, 16384, 2 ** 63):
        assert shim.hs_g1_fft_log2(C.c_uint64(n)) == -1


def test_stage_maps_cover_every_butterfly_once(shim):
    """the ladders of a stage are exactly its butterflies with j != 0, each once, with the twiddle w_n^(j n / 2^s)"""
    for logn in range(1, 8):
        n = 1 << logn
        for s in range(1, logn + 1):
            half = 1 << (s - 1)
            want = {}
            for bf in range(n // 2):
                j = bf & (half - 1)
                if j:
                    want[((bf >> (s - 1)) << s) + j + half] = j * (8192 >> s)
            got = {}
            nl = shim.hs_g1_fft_ladders(logn, s)
            assert nl == len(want) == n // 2 - (n >> s)
            for m in range(nl):
                i1, root = C.c_uint32(), C.c_uint32()
                shim.hs_g1_fft_ladder_index(C.c_uint32(m), s, C.byref(i1), C.byref(root))
                assert i1.value not in got
                got[i1.value] = root.value
            assert got == want
    # the longest transform: the last ladder of the last stage, and every root index stays below 4096 (8192 - it below 8192)
    i1, root = C.c_uint32(), C.c_uint32()
    shim.hs_g1_fft_ladder_index(C.c_uint32(shim.hs_g1_fft_ladders(13, 13) - 1), 13, C.byref(i1), C.byref(root))
    assert (i1.value, root.value) == (8191, 4095)
    assert shim.hs_g1_fft_ladders(13, 13) == 4095 and shim.hs_g1_fft_ladders(13, 1) == 0 and shim.hs_g1_fft_ladders(1, 1) == 0


def test_form_picker_edges(shim):
    q = shim.hs_g1_fft_quad_max_default()
    assert q == 8192
    QUAD, LANE = 0, 1
    form = lambda p, m=q: shim.hs_g1_fft_form(C.c_uint64(p), C.c_uint64(m))
    assert [form(p) for p in (1, q - 1, q, q + 1, 2 ** 40)] == [QUAD, QUAD, QUAD, LANE, LANE]
    assert form(1, 0) == LANE and form(0, 0) == QUAD
    at = lambda logn, count: shim.hs_g1_fft_form_at(logn, C.c_uint64(count), C.c_uint64(q))
    # one and two transforms of 8192 (4095 ladders each in the last stage) are the four-lane form, three are not;
    # at 128 (63 ladders) the hand-over is between 130 and 131 transforms
    assert [at(13, c) for c in (1, 2, 3)] == [QUAD, QUAD, LANE]
    assert [at(7, c) for c in (1, 65, 130, 131)] == [QUAD, QUAD, QUAD, LANE]
    assert at(12, 4) == QUAD and at(12, 5) == LANE
    # the one-term products of the openings: one blob is 8192 products, two are not the four-lane form any more
    assert form(8192) == QUAD and form(2 * 8192) == LANE


def test_chunk_split_edges(shim):
    hdr = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    ch = int(re.search(r"#define CKZG_HIP_DOMAIN_CHUNK_BLOBS (\d+)", hdr).group(1))
    assert 1 <= ch <= 64
    cnt = lambda n: shim.hs_domain_chunk_count(C.c_uint64(n), C.c_uint64(ch))
    size = lambda n, c: shim.hs_domain_chunk_size(C.c_uint64(n), C.c_uint64(ch), C.c_uint64(c))
    assert cnt(0) == 0 and size(0, 0) == 0
    for n in (1, ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 1, 1000):
        sizes = [size(n, c) for c in range(cnt(n))]
        assert sum(sizes) == n and all(1 <= x <= ch for x in sizes) and all(x == ch for x in sizes[:-1]), (n, sizes)
        assert size(n, cnt(n)) == 0
        assert size(n, 0) == min(n, ch)


def test_circulant_source_matches_the_model(shim):
    for N in (4, 16, 4096):
        c = list(range(1, N + 1))
        want = D.circulant(c)
        for t in range(2 * N):
            src = shim.hs_coset_circulant_source(C.c_uint32(t), 0, C.c_uint32(N))   # coset size one: the domain call's map
            assert (c[src] if src >= 0 else 0) == want[t], (N, t)
