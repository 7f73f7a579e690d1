"""What can be said about the stage test shim (tests/native/stage_shim.hip) without a GPU: libstage_shim.so
cross-compiles for gfx950 and exports every ss_* function that tests/test_gpu_rlc_stages.py binds, it is linked from the
product's own object files (the product's entry points are in it), and none of it appears in libckzg_hip.so, whose
export list is still exactly exports.map."""
import os
import re
import subprocess

import pytest

from conftest import HIP_SO, ROOT
from test_gpu_rlc_stages import STAGE_FUNCTIONS, STAGE_SHIM_SO

PKG = os.path.join(ROOT, "c-kzg-4844_amd")


def _defined(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    # (type A: the version node of exports.map itself)
    return {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip() and line.split()[-2] != "A"}


@pytest.fixture(scope="module")
def stage_shim_path():
    if not os.path.exists(STAGE_SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "-j", "8", "libstage_shim.so"])
    return STAGE_SHIM_SO


def test_stage_shim_builds_and_exports_what_the_gpu_module_binds(stage_shim_path):
    names = _defined(stage_shim_path)
    for fn in STAGE_FUNCTIONS:
        assert fn in names, fn
    # linked with the product's objects, without its version script: the stage functions it calls are the product's
    assert "verify_blob_kzg_proof_batch" in names
    assert any("rlc_scalars_enqueue" in s for s in names)


def test_make_all_builds_the_stage_shim():
    with open(os.path.join(PKG, "Makefile")) as f:
        text = f.read()
    all_line = next(line for line in text.splitlines() if line.startswith("all:"))
    assert "libstage_shim.so" in all_line.split()
    rule = next(line for line in text.splitlines() if line.startswith("libstage_shim.so:"))
    assert "$(OBJS)" in rule


def test_the_test_aid_stays_out_of_the_product():
    if not os.path.exists(HIP_SO):
        subprocess.check_call(["make", "-C", PKG, "-j", "8", "libckzg_hip.so"])
    prod = _defined(HIP_SO)
    assert not [s for s in prod if s.startswith("ss_") or "ss_k_" in s]
    with open(os.path.join(PKG, "exports.map")) as f:
        text = f.read()
    listed = set(re.findall(r"^\s+([A-Za-z_][A-Za-z0-9_]*);", text.split("local:")[0], re.M))
    assert listed and prod == listed


def test_the_domain_roots_the_gpu_module_passes_are_the_oracles(oracle):
    """the stages multiply by entries of the table of w^i; the GPU module makes that table from
    w = 7^((R - 1) / 8192).  The oracle's okzg_fr_fft of the unit impulse at index 1 is (w^k), k < 8192, for the w of
    its trusted setup: the two must agree."""
    import ctypes as C

    import rlc_expect as rx
    roots = rx.roots_of_unity()
    n = 8192
    lib = oracle.lib
    one, zero = C.create_string_buffer(32), C.create_string_buffer(32)
    lib.ofr_from_u64(one, C.c_uint64(1))
    lib.ofr_from_u64(zero, C.c_uint64(0))
    inp = C.create_string_buffer(zero.raw + one.raw + zero.raw * (n - 2), 32 * n)
    out = C.create_string_buffer(32 * n)
    f = lib.okzg_fr_fft
    f.restype = C.c_int
    assert f(out, inp, C.c_size_t(n), oracle.sp) == 0
    b = C.create_string_buffer(32)
    for k in range(n):
        lib.ofr_to_bytes(b, C.c_char_p(out.raw[32 * k:32 * k + 32]))
        assert int.from_bytes(b.raw, "big") == roots[k], k
