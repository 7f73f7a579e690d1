"""ckzg_hip_compute_kzg_proof_batch(_device): compute_kzg_proof over n independent (blob, z) items on the GPU, a z on
the evaluation domain included (verify.hip: k_quotient_in_domain).  Every item must come out exactly as the single
compute_kzg_proof call and the CPU oracle do: the consensus-spec vectors in one call, one blob opened at all 4096
domain points, chunk edges with in-domain and random z mixed, invalid items next to valid ones, the device form, the
shard split; and compute_blob_kzg_proof_batch, which lost its host fallback for in-domain challenges."""
import ctypes as C
import random

import pytest

from golden_util import case_names, get_case
from kzg_ctypes import HIP_SO, Kzg

pytestmark = pytest.mark.gpu

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BLOB = 131072
BADARGS = 1


def _fr(v):
    return (v % R).to_bytes(32, "big")


def _brp(i, bits=12):
    return int(format(i, "0%db" % bits)[::-1], 2)


W = pow(7, (R - 1) // 4096, R)
DOMAIN = [_fr(pow(W, _brp(i), R)) for i in range(4096)]   # brp_roots_of_unity: z = DOMAIN[i] opens element i


def _blob(seed):
    rnd = random.Random(seed)
    return b"".join(_fr(rnd.randrange(R)) for _ in range(4096))


@pytest.fixture(scope="module")
def blobs():
    return [_blob(0x5100 + i) for i in range(12)]


def _mixed(blobs, n, seed):
    """n items: every third z a domain point (1, -1 and the last one among them), the others random"""
    rnd = random.Random(seed)
    items = []
    for i in range(n):
        b = blobs[rnd.randrange(len(blobs))]
        if i % 3 == 0:
            j = (0, 1, 4095)[(i // 3) % 3] if i % 9 == 0 else rnd.randrange(4096)
            items.append((b, DOMAIN[j]))
        else:
            items.append((b, _fr(rnd.randrange(R))))
    return items


def _batch(api, items):
    return api.compute_kzg_proof_batch([b for b, _ in items], [z for _, z in items])


def test_golden_vectors_in_one_call(hip):
    items, want = [], []
    for name in case_names("compute_kzg_proof"):
        inp, out = get_case("compute_kzg_proof", name)
        b, z = inp["blob"], inp["z"]
        if b is None or z is None or len(b) != BLOB or len(z) != 32:
            continue
        items.append((b, z))
        want.append((name, out))
    assert len(items) >= 40 and any(o is None for _, o in want)
    # 14 of them open at z = 1 or z = -1, both domain points
    assert sum(1 for b, z in items if z in (DOMAIN[0], DOMAIN[1])) >= 10
    n = len(items)
    proofs, ys, st = (C.create_string_buffer(48 * n), C.create_string_buffer(32 * n), (C.c_uint8 * n)())
    ret = hip.lib.ckzg_hip_compute_kzg_proof_batch(proofs, ys, st, b"".join(b for b, _ in items),
                                                   b"".join(z for _, z in items), C.c_uint64(n), hip.sp)
    assert ret == BADARGS
    for i, (name, out) in enumerate(want):
        if out is None:
            assert st[i] == BADARGS, name
        else:
            assert st[i] == 0, name
            assert proofs.raw[48 * i:48 * i + 48] == out[0], name
            assert ys.raw[32 * i:32 * i + 32] == out[1], name


def test_every_domain_point_of_one_blob(hip, oracle, blobs):
    blob = blobs[0]
    proofs, ys, st = hip.compute_kzg_proof_batch([blob] * 4096, DOMAIN)
    assert st == [0] * 4096
    assert ys == [blob[32 * i:32 * i + 32] for i in range(4096)]
    c = hip.blob_to_kzg_commitment(blob)
    ok, vst = hip.verify_kzg_proof_batch([c] * 4096, DOMAIN, ys, proofs)
    assert vst == [0] * 4096 and all(ok)
    for i in [0, 1, 4095, 2, 3, 2048, 2049] + random.Random(3).sample(range(4, 4095), 9):
        assert (proofs[i], ys[i]) == oracle.compute_kzg_proof(blob, DOMAIN[i]), i


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 600])
def test_chunk_edges_match_single_calls(hip, oracle, blobs, n):
    items = _mixed(blobs, n, n)
    proofs, ys, st = _batch(hip, items)
    assert st == [0] * n
    for i, (b, z) in enumerate(items):
        assert hip.compute_kzg_proof(b, z) == (proofs[i], ys[i]), i
    for i in sorted({0, n - 1, n // 2}):
        assert oracle.compute_kzg_proof(*items[i]) == (proofs[i], ys[i]), i


def _invalid(blobs, n):
    """n mixed items, and the same with invalid items at lanes 0, 63, 64, n - 1: z = r, z = 2^256 - 1, an element = r"""
    good = _mixed(blobs, n, 77 + n)
    bad = list(good)
    rbytes = R.to_bytes(32, "big")
    kinds = [(good[0][0], rbytes), (good[63][0], b"\xff" * 32),
             (good[64][0][:32 * 100] + rbytes + good[64][0][32 * 101:], good[64][1]), (good[n - 1][0], rbytes)]
    lanes = [0, 63, 64, n - 1]
    for lane, item in zip(lanes, kinds):
        bad[lane] = item
    return good, bad, lanes


def test_invalid_items_leave_their_neighbours_alone(hip, blobs):
    n = 300
    good, bad, lanes = _invalid(blobs, n)
    gp, gy, gs = _batch(hip, good)
    assert gs == [0] * n
    bp, by, bs = _batch(hip, bad)
    assert [i for i in range(n) if bs[i]] == lanes and all(bs[i] == BADARGS for i in lanes)
    for i in range(n):
        if i not in lanes:
            assert (bp[i], by[i]) == (gp[i], gy[i]), i
    # the return value, and status may be NULL
    f = hip.lib.ckzg_hip_compute_kzg_proof_batch
    proofs, ys = C.create_string_buffer(48 * n), C.create_string_buffer(32 * n)
    ret = f(proofs, ys, None, b"".join(b for b, _ in bad), b"".join(z for _, z in bad), C.c_uint64(n), hip.sp)
    assert ret == BADARGS
    assert [proofs.raw[48 * i:48 * i + 48] for i in range(n) if i not in lanes] == [bp[i] for i in range(n) if i not in lanes]
    # single calls agree on the verdicts
    for i in lanes:
        with pytest.raises(Exception):
            hip.compute_kzg_proof(*bad[i])


def test_trivial_and_null_arguments(hip):
    f = hip.lib.ckzg_hip_compute_kzg_proof_batch
    assert f(None, None, None, None, None, C.c_uint64(0), hip.sp) == 0
    assert f(None, None, None, None, None, C.c_uint64(1), hip.sp) == BADARGS
    assert hip.compute_kzg_proof_batch([], []) == ([], [], [])


@pytest.fixture(scope="module")
def rt():
    lib = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.hipFree.argtypes = [C.c_void_p]
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return lib


def _device_call(hip, rt, items, host_status=False):
    n = len(items)
    sizes = [48 * n, 32 * n, n, BLOB * n, 32 * n]
    ptrs = []
    try:
        for sz in sizes:
            p = C.c_void_p()
            assert rt.hipMalloc(C.byref(p), max(sz, 1)) == 0
            ptrs.append(p)
        blob_bytes, z_bytes = b"".join(b for b, _ in items), b"".join(z for _, z in items)
        assert rt.hipMemcpy(ptrs[3], C.c_char_p(blob_bytes), len(blob_bytes), 1) == 0
        assert rt.hipMemcpy(ptrs[4], C.c_char_p(z_bytes), len(z_bytes), 1) == 0
        assert rt.hipMemcpy(ptrs[2], C.c_char_p(b"\x07" * n), n, 1) == 0   # (every status byte is written)
        f = hip.lib.ckzg_hip_compute_kzg_proof_batch_device
        if host_status:
            st_host = (C.c_uint8 * n)()
            return f(ptrs[0], ptrs[1], st_host, ptrs[3], ptrs[4], C.c_uint64(n), hip.sp)
        ret = f(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], C.c_uint64(n), hip.sp)
        out = []
        for p, sz in zip(ptrs[:3], sizes[:3]):
            h = C.create_string_buffer(sz)
            assert rt.hipMemcpy(h, p, sz, 2) == 0
            out.append(h.raw)
        return ret, [out[0][48 * i:48 * i + 48] for i in range(n)], [out[1][32 * i:32 * i + 32] for i in range(n)], list(out[2])
    finally:
        for p in ptrs:
            rt.hipFree(p)


def test_device_form_matches_host_form(hip, rt, blobs):
    n = 300
    good, bad, lanes = _invalid(blobs, n)
    hp, hy, hs = _batch(hip, bad)
    ret, dp, dy, ds = _device_call(hip, rt, bad)
    assert ret == 0   # invalid items are reported through d_status only
    assert ds == hs and [i for i in range(n) if ds[i]] == lanes
    for i in range(n):
        if i not in lanes:
            assert (dp[i], dy[i]) == (hp[i], hy[i]), i
    # a host pointer among the arguments: C_KZG_BADARGS, nothing launched
    assert _device_call(hip, rt, good[:4], host_status=True) == BADARGS
    f = hip.lib.ckzg_hip_compute_kzg_proof_batch_device
    assert f(None, None, None, None, None, C.c_uint64(0), hip.sp) == 0


def test_shard_split_over_two_replicas(hip, blobs):
    items = _mixed(blobs, 700, 11)
    want = _batch(hip, items)
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        assert _batch(api, items) == want
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


def test_blob_proof_batch_matches_single_calls(hip, oracle, blobs):
    """past a chunk edge (256): the batch path whose in-domain challenges used to leave for the host"""
    n = 300
    bl = [_fr(i) + blobs[i % len(blobs)][32:] for i in range(n)]   # 300 distinct blobs
    cm = [hip.blob_to_kzg_commitment(b) for b in bl]
    proofs = C.create_string_buffer(48 * n)
    st = (C.c_uint8 * n)()
    ret = hip.lib.ckzg_hip_compute_blob_kzg_proof_batch(proofs, st, b"".join(bl), b"".join(cm), C.c_uint64(n), hip.sp)
    assert ret == 0 and list(st) == [0] * n
    for i in range(n):
        assert hip.compute_blob_kzg_proof(bl[i], cm[i]) == proofs.raw[48 * i:48 * i + 48], i
    for i in (0, 257):
        assert oracle.compute_blob_kzg_proof(bl[i], cm[i]) == proofs.raw[48 * i:48 * i + 48], i
