"""The throughput accumulate loop on 30-bit limbs (msm.hip: msm_sum_pairs30, g1_30.hpp) on the device.

1. Commitment batches through the C-ABI over the library's default 10-bit table, at the smallest batch that takes the
   throughput form of k_msm_accumulate and at one blob more (the bound comes from gs_msm_plan + run_msm's conditions,
   asserted below): random blobs, the edge-digit blob, the all-zero blob and a blob with an element >= r, against the
   oracle and against the 28-bit loop the kernel had before (libckzg_hip_ab.so with CKZG_HIP_MSM_LOOP28=1).
2. The equal-x fallback.  No blob can make a lane of the commitment meet an entry with its accumulator's x: within a
   half the digits are too small for one entry to equal a sum of others, across phi it would take a GLV lattice vector
   shorter than the shortest, and the setup's bases are unrelated.  So the fallback is driven the way
   tests/test_gpu_g1_stages.py drives the 28-bit branches: a table over chosen bases with a_(i+256) = a_i, and digit
   vectors that make one lane add an entry to itself (doubling) and another add an entry to its negative
   (cancellation) in every window, through the same throughput form, against the sum as an integer mod r."""
import ctypes as C
import hashlib
import os
import random

import pytest

import g1_expect as gx
from g1_expect import R
from conftest import ROOT
from test_gpu_g1_stages import (shim, src, device_table, from_digits, digit_kinds, run_form)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

AB_SO = os.path.join(ROOT, "c-kzg-4844_amd", "libckzg_hip_ab.so")


def rand_blob(seed, i):
    out = bytearray()
    for j in range(4096):
        out += b"\x00" + hashlib.sha256(b"%d|%d|%d" % (seed, i, j)).digest()[:31]
    return bytes(out)


def edge_blob():
    vals = [0, 1, R - 1, R - 2, 2 ** 254, (2 ** 255 - 19) % R, (R - 1) // 2, 0x8000800080008000 << 128]
    blob = bytearray()
    for j in range(4096):
        v = vals[j % len(vals)] if j < 64 else int.from_bytes(hashlib.sha256(b"e%d" % j).digest(), "big") % R
        blob += v.to_bytes(32, "big")
    return bytes(blob)


def smallest_throughput_batch(shim, npoints, wbits):
    """the smallest nvec whose launch is not run_msm's form A, i.e. runs k_msm_accumulate<256, false>"""
    for nvec in range(1, 200):
        ppb, bpv = shim.plan(npoints, wbits, nvec)
        if run_form(ppb, bpv, nvec) != "A":
            return nvec
    pytest.fail("no batch below 200 takes the throughput form")


@pytest.fixture(scope="module")
def hip_loop28():
    """the A/B twin of the product with the 28-bit loop selected (read once, at the first launch)"""
    from kzg_ctypes import Kzg
    if not os.path.exists(AB_SO):
        pytest.fail("libckzg_hip_ab.so is not built: run python -c 'import __graft_entry__ as g; g.build()'")
    if os.environ.get("CKZG_HIP_SO"):
        pytest.skip("variant build under test: the twin is the product's")
    os.environ["CKZG_HIP_MSM_LOOP28"] = "1"
    api = Kzg(AB_SO, "", precompute=0)
    yield api
    api.close()


def device_commit(api, blobs):
    rt = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipFree.argtypes = [C.c_void_p]
    n, raw = len(blobs), b"".join(blobs)
    bufs = []
    for nbytes in (len(raw), 48 * n, n):
        q = C.c_void_p()
        assert rt.hipMalloc(C.byref(q), nbytes) == 0
        bufs.append(q)
    d_blobs, d_out, d_st = bufs
    try:
        assert rt.hipMemcpy(d_blobs, C.cast(C.c_char_p(raw), C.c_void_p), len(raw), 1) == 0
        f = api.lib.ckzg_hip_blob_to_kzg_commitment_batch_device
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        rc = f(d_out, d_st, d_blobs, n, api.sp)
        out, st = C.create_string_buffer(48 * n), C.create_string_buffer(n)
        assert rt.hipMemcpy(out, d_out, 48 * n, 2) == 0 and rt.hipMemcpy(st, d_st, n, 2) == 0
    finally:
        for q in bufs:
            rt.hipFree(q)
    return rc, [out.raw[48 * i:48 * i + 48] for i in range(n)], list(st.raw)


@pytest.fixture(scope="module")
def blob_set(oracle):
    """the blobs of both batches and their commitments by the oracle, computed once"""
    bad = bytearray(rand_blob(30, 99))
    bad[32 * 4095:32 * 4096] = R.to_bytes(32, "big")
    blobs = [rand_blob(30, 0), edge_blob(), bytes(131072), bytes(bad)] + [rand_blob(30, i) for i in range(1, 4)]
    want = [None if i == 3 else oracle.blob_to_kzg_commitment(b) for i, b in enumerate(blobs)]
    return blobs, want


def test_the_bound_is_run_msms(shim):
    n = smallest_throughput_batch(shim, 4096, 10)
    ppb, bpv = shim.plan(4096, 10, n)
    pairs = 2 * gx.twin_for(10) * 4096
    # run_msm: form A needs bpv > 8, ppb <= 1024 and all workgroups resident (nvec * bpv <= 512)
    assert n >= 2 and run_form(*shim.plan(4096, 10, n - 1), n - 1) == "A"
    assert not (8 < bpv <= 512 and ppb <= 1024 and n * bpv <= 512) and bpv == (pairs + ppb - 1) // ppb
    assert n + 1 <= 7   # blob_set holds seven blobs


@pytest.mark.parametrize("extra", [0, 1])
def test_commitments_match_oracle_and_the_28_bit_loop(hip, hip_loop28, shim, blob_set, extra):
    blobs, want = blob_set
    n = smallest_throughput_batch(shim, 4096, 10) + extra
    assert 5 <= n <= len(blobs)
    rc, got, st = device_commit(hip, blobs[:n])
    assert rc == 0 and st == [1 if i == 3 else 0 for i in range(n)]
    rc28, got28, st28 = device_commit(hip_loop28, blobs[:n])
    assert rc28 == 0 and st28 == st
    for i in range(n):
        if i != 3:
            assert got[i] == want[i], "blob %d differs from the oracle" % i
            assert got28[i] == want[i], "blob %d: the 28-bit loop differs from the oracle" % i
    assert got[2] == gx.INF48 and got == got28


def test_equal_x_in_a_lane_takes_the_fallback(shim, src):
    npoints, c = 512, 4
    rnd = random.Random(3030)
    a = [rnd.randrange(1, R) for _ in range(npoints)]
    a[272], a[273] = a[16], a[17]           # lane 16 reads bases 16 and 272, lane 17 reads 17 and 273
    table = device_table(shim, src, a, c)
    half, twin = 1 << (c - 1), gx.twin_for(c)
    pairs = 2 * twin * npoints
    event = [0] * pairs
    for w in range(2 * twin):
        d = rnd.choice([v for v in range(-half, half + 1) if v])
        event[w * npoints + 16] = event[w * npoints + 272] = d     # E + E
        event[w * npoints + 17], event[w * npoints + 273] = d, -d  # E - E, and the lane goes on from infinity
    only_cancel = [0] * pairs                                      # every lane ends at infinity
    for w in range(2 * twin):
        only_cancel[w * npoints + 17], only_cancel[w * npoints + 273] = half, -half
    mixed = digit_kinds(npoints, c, rnd)[0]
    for w in range(0, 2 * twin, 3):
        mixed[w * npoints + 272] = mixed[w * npoints + 16] or 1
        mixed[w * npoints + 16] = mixed[w * npoints + 272]
    kinds = [event, only_cancel, mixed] + digit_kinds(npoints, c, rnd)[:2]
    want = [src.compressed(gx.digit_sum(d, a, npoints, c)) for d in kinds]
    assert want[1] == gx.INF48 and want[0] != gx.INF48
    n0 = smallest_throughput_batch(shim, npoints, c)
    for nvec in (n0, n0 + 1):
        ppb, bpv = shim.plan(npoints, c, nvec)
        assert run_form(ppb, bpv, nvec) != "A"
        # both reads of a window fall into one block (hence one lane) in at least one window
        assert any((w * npoints + 16) // ppb == (w * npoints + 272) // ppb for w in range(2 * twin))
        order = [v % len(kinds) for v in range(nvec)]
        got = from_digits(shim, table, npoints, c, kinds, order)
        for v, j in enumerate(order):
            assert got[v] == want[j], "nvec %d, vector %d (kind %d)" % (nvec, v, j)
