"""ckzg_hip_compute_kzg_proof_batch(_device) without a GPU: both symbols are declared and exported, a settings struct
without GPU state gives C_KZG_ERROR (no CPU fallback), the in-domain quotient kernel is in the product with no scratch,
and its algorithm (verify.hip: k_quotient_in_domain, fr29.hpp: ev29::quotient_in_domain), replayed thread by thread on
the host through libhost_shim.so, gives the quotient of eip4844.c:441-481 computed with Python integers."""
import ctypes as C
import importlib.util
import os
import random
import subprocess

import pytest

from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, KZGSettings
from test_abi_exports import declared_symbols

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NEW = ("ckzg_hip_compute_kzg_proof_batch", "ckzg_hip_compute_kzg_proof_batch_device")


def test_symbols_declared_and_exported():
    names = declared_symbols()
    for n in NEW:
        assert n in names, n
    exports = open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    lib = C.CDLL(HIP_SO)
    for n in NEW:
        assert "    %s;\n" % n in exports, n
        assert hasattr(lib, n), n


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    lib = C.CDLL(HIP_SO)
    s = KZGSettings()
    blob, z = bytes(131072), (1).to_bytes(32, "big")
    proof, y, st = C.create_string_buffer(48), C.create_string_buffer(32), (C.c_uint8 * 1)()
    f = lib.ckzg_hip_compute_kzg_proof_batch
    f.restype = C.c_int
    assert f(proof, y, st, blob, z, C.c_uint64(1), C.byref(s)) == 2
    assert f(None, None, None, None, None, C.c_uint64(0), C.byref(s)) == 2
    g = lib.ckzg_hip_compute_kzg_proof_batch_device
    g.restype = C.c_int
    assert g(None, None, None, None, None, C.c_uint64(1), C.byref(s)) == 2
    # the single call is a batch of one: the same answer
    h = lib.compute_kzg_proof
    h.restype = C.c_int
    assert h(proof, y, blob, z, C.byref(s)) == 2


def test_in_domain_kernel_present_without_scratch():
    if os.environ.get("CKZG_HIP_SO"):
        pytest.skip("sanitizer / variant build: the budget is the product's")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    table = {k.split(":", 1)[1]: v for k, v in m.collect().items()}
    assert "k_quotient_in_domain" in table, sorted(table)
    assert table["k_quotient_in_domain"]["scratch"] == 0, table["k_quotient_in_domain"]
    assert table["k_quotient_in_domain"]["vgpr"] <= 256, table["k_quotient_in_domain"]


def _brp(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    return C.CDLL(SHIM_SO)


@pytest.mark.parametrize("m,kind", [(0, "random"), (1, "random"), (2, "random"), (1234, "random"), (4095, "random"),
                                    (7, "extreme"), (2048, "constant"), (3, "one_hot")])
def test_in_domain_quotient_replay(shim, m, kind):
    """z = brp_roots[m] (m = 0: z = 1, m = 1: z = -1), y = p_m; q_i = (p_i - y)/(w_i - z) for i != m and
    q_m = sum_{i != m} (p_i - y) w_i / (z (z - w_i)), as eip4844.c:441-481 computes them"""
    rnd = random.Random(1000 + m)
    r256 = pow(2, 256, R)
    w = pow(7, (R - 1) // 4096, R)
    roots = [pow(w, _brp(i, 12), R) for i in range(4096)]
    if kind == "random":
        poly = [rnd.randrange(R) for _ in range(4096)]
    elif kind == "extreme":
        poly = [R - 1 if i % 2 else 0 for i in range(4096)]
    elif kind == "constant":
        poly = [12345] * 4096            # a constant polynomial: the quotient is zero
    else:
        poly = [1 if i == 3 else 0 for i in range(4096)]
    z, y = roots[m], poly[m]
    want = [0] * 4096
    for i in range(4096):
        if i != m:
            want[i] = (poly[i] - y) * pow((roots[i] - z) % R, -1, R) % R
    want[m] = sum((poly[i] - y) * roots[i] % R * pow(z * (z - roots[i]) % R, -1, R)
                  for i in range(4096) if i != m) % R
    pb = b"".join((p * r256 % R).to_bytes(32, "little") for p in poly)
    rb = b"".join((x * r256 % R).to_bytes(32, "little") for x in roots)
    out = C.create_string_buffer(4096 * 32)
    shim.hs_fr29_quotient_in_domain(out, pb, C.c_int(m), rb)
    got = [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(4096)]
    assert got[m] == want[m]
    assert got == want
    if kind == "constant":
        assert not any(got)
