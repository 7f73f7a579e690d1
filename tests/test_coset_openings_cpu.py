"""ckzg_hip_compute_coset_kzg_proofs_batch(_device) without a GPU: the index maps and the column-sum split of
csrc/g1_fft_plan.hpp for every coset size, through libhost_shim.so, against the model (tests/coset_expect.py); the two
symbols are declared, exported and bound; a settings struct without GPU state gives C_KZG_ERROR (no CPU fallback); a
coset size above 64 and NULL arguments give C_KZG_BADARGS before anything else."""
import ctypes as C
import os
import re
import subprocess

import pytest

import coset_expect as E
import domain_expect as D
from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, KZGSettings
from test_abi_exports import declared_symbols

NEW = ("ckzg_hip_compute_coset_kzg_proofs_batch", "ckzg_hip_compute_coset_kzg_proofs_batch_device")
HDR = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    assert hasattr(lib, "hs_coset_circulant_source")
    for n in ("hs_coset_proofs_per_blob", "hs_coset_colsum_radix", "hs_coset_colsum_parts"):
        getattr(lib, n).restype = C.c_uint32
    return lib


# ---- csrc/g1_fft_plan.hpp ----

def test_sizes(shim):
    assert shim.hs_coset_max_log() == 6 == int(re.search(r"#define CKZG_HIP_COSET_MAX_LOG2\s+(\d+)", HDR).group(1))
    assert [shim.hs_coset_proofs_per_blob(e) for e in range(7)] == [8192 >> e for e in range(7)]


@pytest.mark.parametrize("e", range(7))
def test_circulant_source_matches_the_model(shim, e):
    for N in (64 << max(e - 5, 0), 4096):   # a small blob on which the model was checked against the definition, and the product's
        if (1 << e) > N // 2:
            continue
        p = list(range(1, N + 1))
        flat = [x for col in E.circulant_columns(p, 1 << e) for x in col]
        got = [shim.hs_coset_circulant_source(C.c_uint32(t), e, C.c_uint32(N)) for t in range(2 * N)]
        assert [p[s] if s >= 0 else 0 for s in got] == flat
        assert got == [E.circulant_source(t, e, N) for t in range(2 * N)]
        assert sorted(s for s in got if s >= 0) == list(range(1 << e, N))
    if e == 0:   # the single-point form's vector: v[0] = c[N-1], v[1 .. N+1] = 0, v[N+2+j] = c[1+j] for j = 0 .. N-3
        assert [shim.hs_coset_circulant_source(C.c_uint32(t), 0, C.c_uint32(4096)) for t in range(8192)] == \
            [4095 if t == 0 else t - 4097 if t >= 4098 else -1 for t in range(8192)]


@pytest.mark.parametrize("e", range(7))
def test_setup_source_matches_the_model(shim, e):
    l = 1 << e
    for N in (64, 4096):
        if l > N // 2:
            continue
        k = N // l
        got = [shim.hs_coset_setup_source(C.c_uint32(t), e, C.c_uint32(N)) for t in range(2 * N)]
        assert got == [E.setup_source(t, e, N) for t in range(2 * N)]
        s = 5
        xs = [x for col in E.setup_columns(s, N, l) for x in col]
        assert [pow(s, i, D.R) if i >= 0 else 0 for i in got] == xs
        live = [i for i in got if i >= 0]
        assert len(live) == len(set(live)) == l * (k - 1) and min(live) == 0 and max(live) == N - l - 1
    if e == 0:   # the single-point form's gather: g1_values_monomial[4094 - t] for t <= 4094
        got = [shim.hs_coset_setup_source(C.c_uint32(t), 0, C.c_uint32(4096)) for t in range(8192)]
        assert got == [4094 - t if t <= 4094 else -1 for t in range(8192)]


def test_column_sum_split(shim):
    radix = shim.hs_coset_colsum_radix()
    assert radix == 8
    for e in range(7):
        l, parts = 1 << e, shim.hs_coset_colsum_parts(e)
        assert parts >= 1 and l % parts == 0
        if l <= radix:
            assert parts == 1
        else:
            assert l // parts == radix and parts <= radix   # no pass is deeper than the radix
        # the two passes read every column exactly once: pass one column part + j parts into `part`, pass two the parts
        if parts > 1:
            seen = sorted(part + j * parts for part in range(parts) for j in range(l // parts))
            assert seen == list(range(l))


# ---- the symbols ----

def test_symbols_declared_exported_and_bound():
    names = declared_symbols()
    exports = open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    binding = open(os.path.join(ROOT, "c-kzg-4844_amd", "ckzg.py")).read()
    lib = C.CDLL(HIP_SO)
    for n in NEW:
        assert n in names, n
        assert "    %s;\n" % n in exports, n
        assert hasattr(lib, n), n
    assert '"%s"' % NEW[0] in binding and "def compute_coset_kzg_proofs_batch(self, blobs, log2_coset, want_evals=False)" in binding
    assert re.search(r"#define CKZG_HIP_COSET_CHUNK_BLOBS\s+16\b", HDR)
    assert re.search(r"#define CKZG_HIP_COSET_MAX_LOG2\s+6\b", HDR)


def _fns():
    lib = C.CDLL(HIP_SO)
    g, h = (getattr(lib, n) for n in NEW)
    for x in (g, h):
        x.restype = C.c_int
        x.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    return g, h


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    s = KZGSettings()
    proofs, st, blob = C.create_string_buffer(128 * 48), (C.c_uint8 * 1)(), C.create_string_buffer(131072)
    for fn in _fns():
        for e in (0, 3, 6):
            assert fn(proofs, None, st, blob, 1, e, C.byref(s)) == 2
        assert fn(None, None, None, None, 0, 0, C.byref(s)) == 2
    assert proofs.raw == bytes(128 * 48)


def test_bad_arguments_are_rejected_before_any_gpu_work():
    """(a zeroed settings struct: a check that came after the first look at the device would answer C_KZG_ERROR)"""
    s = KZGSettings()
    proofs, ev, blob = C.create_string_buffer(48), C.create_string_buffer(32), C.create_string_buffer(32)
    for fn in _fns():
        assert fn(None, None, None, blob, 1, 3, C.byref(s)) == 1
        assert fn(proofs, None, None, None, 1, 3, C.byref(s)) == 1
        for e in (7, 8, 13, 64, 2 ** 32 - 1):
            assert fn(proofs, ev, None, blob, 1, e, C.byref(s)) == 1, e
            assert fn(None, None, None, None, 0, e, C.byref(s)) == 1, e
    assert proofs.raw == bytes(48) and ev.raw == bytes(32)
