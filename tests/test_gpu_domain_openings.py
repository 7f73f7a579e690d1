"""ckzg_hip_compute_domain_kzg_proofs_batch(_device): a blob opened at every point of the evaluation domain in one call
(c-kzg-4844_amd/csrc/g1_fft.hip; the layout's model is tests/domain_expect.py).  The reference is never the call under
test: it is ckzg_hip_compute_kzg_proof_batch at the 4096 z_j, which the consensus vectors pin, plus the CPU oracle on
sampled indices, closed forms for the edge polynomials, and the batch verification as an independent soundness check."""
import ctypes as C
import random
import re

import pytest

import domain_expect as D
from conftest import ROOT
from kzg_ctypes import HIP_SO, Kzg
from test_gpu_locate import G1
from test_gpu_point_openings import BLOB, DOMAIN, _blob, _fr, rt  # noqa: F401  (rt: the HIP runtime fixture)

pytestmark = pytest.mark.gpu
R = D.R
BADARGS = 1
INF48 = b"\xc0" + bytes(47)
CHUNK = int(re.search(r"#define CKZG_HIP_DOMAIN_CHUNK_BLOBS (\d+)", open(ROOT + "/include/ckzg_hip.h").read()).group(1))
PER = 4096 * 48


def test_the_domain_points_of_the_test(hip):
    assert DOMAIN == D.domain_points()


class Reference:
    """the 4096 openings of a blob by ckzg_hip_compute_kzg_proof_batch, once per distinct blob"""

    def __init__(self, hip):
        self.hip, self.cache = hip, {}

    def __call__(self, blob):
        if blob not in self.cache:
            proofs, ys, st = self.hip.compute_kzg_proof_batch([blob] * 4096, DOMAIN)
            assert st == [0] * 4096
            # that call's ys are the blob's own elements: this pins the order of the z_j
            assert ys == [blob[32 * j:32 * j + 32] for j in range(4096)]
            self.cache[blob] = proofs
        return self.cache[blob]


@pytest.fixture(scope="module")
def ref(hip):
    return Reference(hip)


@pytest.fixture(scope="module")
def two_blobs():
    return [_blob(0xD0 + i) for i in range(2)]


def _compress(g1, p):
    out = C.create_string_buffer(48)
    g1.o.og1_compress(out, p)
    return out.raw


def test_one_random_blob(hip, oracle, ref, two_blobs):
    blob = two_blobs[0]
    proofs, st = hip.compute_domain_kzg_proofs_batch([blob])
    assert st == [0]
    want = ref(blob)
    assert proofs[0] == want
    for j in [0, 1, 4095] + random.Random(5).sample(range(2, 4095), 5):
        assert oracle.compute_kzg_proof(blob, DOMAIN[j]) == (proofs[0][j], blob[32 * j:32 * j + 32]), j


def test_edge_polynomials(hip, ref):
    g1 = G1()
    a, b = 0x1234567, random.Random(9).randrange(R)
    zero, const, line = D.blob_of_poly([]), D.blob_of_poly([a]), D.blob_of_poly([a, b])
    assert zero == bytes(BLOB) and const == _fr(a) * 4096
    monomials = [D.blob_of_poly([0] * e + [1]) for e in (4095, 4094, 1)]   # the only terms in circulant slots 0, 8191, 4098
    full = D.blob_of_poly([random.Random(10).randrange(R) for _ in range(4095)] + [R - 1])
    blobs = [zero, const, line] + monomials + [full]
    proofs, st = hip.compute_domain_kzg_proofs_batch(blobs)
    assert st == [0] * len(blobs)
    assert proofs[0] == [INF48] * 4096 and proofs[1] == [INF48] * 4096
    assert proofs[2] == [_compress(g1, g1.mul(g1.gen, b))] * 4096
    for i in range(2, len(blobs)):
        assert proofs[i] == ref(blobs[i]), i
    # X: the quotient at any point is 1, the proof is G itself
    assert proofs[5] == [_compress(g1, g1.gen)] * 4096


def test_a_bad_blob_in_a_batch(hip, ref, two_blobs):
    bad = two_blobs[0][:32 * 77] + R.to_bytes(32, "big") + two_blobs[0][32 * 78:]
    proofs, st = hip.compute_domain_kzg_proofs_batch([two_blobs[0], bad, two_blobs[1]])
    assert st == [0, 1, 0]
    assert proofs[0] == ref(two_blobs[0]) and proofs[2] == ref(two_blobs[1])
    f = hip.lib.ckzg_hip_compute_domain_kzg_proofs_batch
    f.restype = C.c_int
    out = C.create_string_buffer(3 * PER)
    assert f(out, None, two_blobs[0] + bad + two_blobs[1], C.c_uint64(3), hip.sp) == BADARGS   # status may be NULL
    assert out.raw[:PER] == b"".join(ref(two_blobs[0])) and out.raw[2 * PER:] == b"".join(ref(two_blobs[1]))
    assert f(out, None, bad, C.c_uint64(1), hip.sp) == BADARGS
    # n = 0, NULL arguments
    assert f(None, None, None, C.c_uint64(0), hip.sp) == 0
    assert hip.compute_domain_kzg_proofs_batch([]) == ([], [])
    assert f(None, None, two_blobs[0], C.c_uint64(1), hip.sp) == BADARGS
    assert f(out, None, None, C.c_uint64(1), hip.sp) == BADARGS


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_chunk_edge(hip, ref, two_blobs, n):
    rnd = random.Random(n)
    pick = [rnd.randrange(2) for _ in range(n)]
    pick[0], pick[n - 1] = 0, 1
    if n > CHUNK:
        pick[CHUNK - 1], pick[CHUNK] = 1, 0
    proofs, st = hip.compute_domain_kzg_proofs_batch([two_blobs[i] for i in pick])
    assert st == [0] * n
    for i in range(n):
        assert proofs[i] == ref(two_blobs[pick[i]]), i


def _device_call(hip, rt, blobs, host_status=False):
    n = len(blobs)
    sizes = [PER * n, n, BLOB * n]
    ptrs = []
    try:
        for sz in sizes:
            p = C.c_void_p()
            assert rt.hipMalloc(C.byref(p), max(sz, 1)) == 0
            ptrs.append(p)
        data = b"".join(blobs)
        assert rt.hipMemcpy(ptrs[2], C.c_char_p(data), len(data), 1) == 0
        assert rt.hipMemcpy(ptrs[1], C.c_char_p(b"\x07" * n), n, 1) == 0   # (every status byte is written)
        f = hip.lib.ckzg_hip_compute_domain_kzg_proofs_batch_device
        f.restype = C.c_int
        if host_status:
            return f(ptrs[0], (C.c_uint8 * n)(), ptrs[2], C.c_uint64(n), hip.sp)
        ret = f(ptrs[0], ptrs[1], ptrs[2], C.c_uint64(n), hip.sp)
        out, st = C.create_string_buffer(sizes[0]), C.create_string_buffer(n)
        assert rt.hipMemcpy(out, ptrs[0], sizes[0], 2) == 0 and rt.hipMemcpy(st, ptrs[1], n, 2) == 0
        return ret, out.raw, list(st.raw)
    finally:
        for p in ptrs:
            rt.hipFree(p)


def test_device_form(hip, rt, ref, two_blobs):  # noqa: F811
    bad = two_blobs[1][:-32] + b"\xff" * 32
    blobs = [two_blobs[1], bad, two_blobs[0]]
    hp, hs = hip.compute_domain_kzg_proofs_batch(blobs)
    ret, out, st = _device_call(hip, rt, blobs)
    assert ret == 0 and st == hs == [0, 1, 0]   # invalid blobs are reported through d_status only
    assert out[:PER] == b"".join(hp[0]) == b"".join(ref(two_blobs[1]))
    assert out[2 * PER:] == b"".join(hp[2]) == b"".join(ref(two_blobs[0]))
    assert _device_call(hip, rt, blobs[:1], host_status=True) == BADARGS   # a host pointer: nothing launched
    f = hip.lib.ckzg_hip_compute_domain_kzg_proofs_batch_device
    f.restype = C.c_int
    assert f(None, None, None, C.c_uint64(0), hip.sp) == 0
    assert f(None, None, None, C.c_uint64(1), hip.sp) == BADARGS


def test_two_replicas(hip, two_blobs):
    blobs = [two_blobs[0], two_blobs[1], two_blobs[0]]
    want = hip.compute_domain_kzg_proofs_batch(blobs)
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        assert api.compute_domain_kzg_proofs_batch(blobs) == want
    finally:
        api.close()
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


def test_lazy_state(hip, ref, two_blobs):
    """nothing is built or allocated at load time: the tables' bytes are those of a load that never opens a domain, and
    the first call on fresh settings is right"""
    def table_bytes(k):
        f = k.lib.ckzg_hip_table_bytes
        f.restype = C.c_uint64
        return f(k.sp)

    # the load's tables depend on the options alone: a second load with the same options that never opens a domain
    # holds the same bytes
    opts = {"commit_wbits": 8, "proof_wbits": 6}
    other = Kzg(HIP_SO, "", precompute=0, options=opts)
    try:
        untouched = table_bytes(other)
    finally:
        other.close()
    api = Kzg(HIP_SO, "", precompute=0, options=opts)
    try:
        before = table_bytes(api)
        assert before == untouched > 0
        proofs, st = api.compute_domain_kzg_proofs_batch([two_blobs[1]])
        assert st == [0] and proofs[0] == ref(two_blobs[1])
        assert table_bytes(api) == before
        assert api.compute_domain_kzg_proofs_batch([two_blobs[0]])[0][0] == ref(two_blobs[0])
    finally:
        api.close()
        for k, v in ((b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


def test_every_proof_verifies(hip, two_blobs):
    """independent of every computation above: the 4096 (C, z_j, y_j, pi_j) pass the batch check, in one range check"""
    blob = two_blobs[1]
    proofs, st = hip.compute_domain_kzg_proofs_batch([blob])
    c = hip.blob_to_kzg_commitment(blob)
    ys = [blob[32 * j:32 * j + 32] for j in range(4096)]
    ok, vst, stats = hip.verify_kzg_proof_batch_locate([c] * 4096, DOMAIN, ys, proofs[0])
    assert vst == [0] * 4096 and all(ok)
    assert stats[0] == 1
    # and a wrong one among them is found
    swapped = list(proofs[0])
    swapped[100], swapped[101] = swapped[101], swapped[100]
    ok, vst, stats = hip.verify_kzg_proof_batch_locate([c] * 4096, DOMAIN, ys, swapped)
    assert [j for j in range(4096) if not ok[j]] == [100, 101]
