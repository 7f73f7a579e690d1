"""ckzg_hip_compute_coset_kzg_proofs_batch(_device): a blob opened on every coset of 2^e points of the extended domain
(c-kzg-4844_amd/csrc/g1_fft.hip; the layout's model is tests/coset_expect.py).  The reference is never the call under
test.  e = 0 hangs on ckzg_hip_compute_domain_kzg_proofs_batch, ckzg_hip_compute_kzg_proof_batch and the CPU oracle;
e = 6 on compute_cells_and_kzg_proofs (library and oracle) and verify_cell_kzg_proof_batch; every size in between on the
one below it, by pi_e[c] = [1 / (2a)] (pi_{e-1}[2c] - pi_{e-1}[2c+1]) in the oracle's G1 arithmetic, ALL 8064 relations;
e = 3 also by the definition of the quotient on the setup file's points; closed forms for the edge polynomials."""
import ctypes as C
import random
import re

import pytest

import coset_expect as E
import domain_expect as D
from conftest import ROOT
from kzg_ctypes import HIP_SO, TRUSTED_SETUP, Kzg
from test_gpu_locate import G1, G48
from test_gpu_point_openings import BLOB, _blob, _fr, rt  # noqa: F401  (rt: the HIP runtime fixture)

pytestmark = pytest.mark.gpu
R = D.R
BADARGS = 1
INF48 = b"\xc0" + bytes(47)
HDR = open(ROOT + "/include/ckzg_hip.h").read()
CHUNK = int(re.search(r"#define CKZG_HIP_COSET_CHUNK_BLOBS (\d+)", HDR).group(1))
ZS = E.ext_domain_points()            # brp_roots_of_unity of the 8192-point domain, integers
EXT = [_fr(z) for z in ZS]


def _m(e):
    return 8192 >> e


@pytest.fixture(scope="module")
def g1():
    return G1()


@pytest.fixture(scope="module")
def two_blobs():
    return [_blob(0xC05E + i) for i in range(2)]


class Levels:
    """(proofs, evals) of one blob at every coset size, one call per (blob, e)"""

    def __init__(self, hip):
        self.hip, self.cache = hip, {}

    def __call__(self, blob, e):
        if (blob, e) not in self.cache:
            proofs, evals, st = self.hip.compute_coset_kzg_proofs_batch([blob], e, want_evals=True)
            assert st == [0] and len(proofs[0]) == _m(e) and len(evals[0]) == 8192 * 32
            self.cache[(blob, e)] = (proofs[0], evals[0])
        return self.cache[(blob, e)]


@pytest.fixture(scope="module")
def levels(hip):
    return Levels(hip)


def _jac(g1, b48):
    aff, out = C.create_string_buffer(96), C.create_string_buffer(144)
    assert g1.o.og1_uncompress(aff, b48) == 0
    g1.o.og1_from_affine(out, aff)
    return out.raw


def _compress(g1, p):
    out = C.create_string_buffer(48)
    g1.o.og1_compress(out, p)
    return out.raw


def _ladder_at(g1, size_one, e, c):
    """proof c at coset size 2^e from the 2^e proofs at size one below it: 2^e - 1 relations"""
    level = [_jac(g1, b) for b in size_one[c << e:(c + 1) << e]]
    for k in range(1, e + 1):
        nxt = []
        for i in range(len(level) // 2):
            a = pow(ZS[((c << (e - k)) + i) << k], 1 << (k - 1), R)
            nxt.append(g1.mul(g1.add(level[2 * i], g1.neg(level[2 * i + 1])), pow(2 * a, -1, R)))
        level = nxt
    return _compress(g1, level[0])


def _ladder(g1, lower, e):
    """the proofs at coset size 2^e from the bytes of those at 2^(e-1), in the oracle's arithmetic"""
    l, out = 1 << e, []
    pts = [_jac(g1, b) for b in lower]
    for c in range(_m(e)):
        a = pow(ZS[c * l], l // 2, R)
        diff = g1.add(pts[2 * c], g1.neg(pts[2 * c + 1]))
        out.append(_compress(g1, g1.mul(diff, pow(2 * a, -1, R))))
    return out


# ---- anchors ----

def test_size_one_is_compute_kzg_proof_at_all_8192_points(hip, oracle, levels, two_blobs):
    blob = two_blobs[0]
    proofs, evals = levels(blob, 0)
    inner, st = hip.compute_domain_kzg_proofs_batch([blob])
    assert st == [0] and proofs[:4096] == inner[0]
    assert evals[:BLOB] == blob
    outer, ys, st = hip.compute_kzg_proof_batch([blob] * 4096, EXT[4096:])
    assert st == [0] * 4096
    assert b"".join(ys) == evals[BLOB:]            # this pins the order of the outer points
    assert proofs[4096:] == outer
    for j in [0, 4095, 4096, 8191] + random.Random(5).sample(range(8192), 5):
        assert oracle.compute_kzg_proof(blob, EXT[j]) == (proofs[j], evals[32 * j:32 * j + 32]), j


def test_size_64_is_compute_cells_and_kzg_proofs(hip, oracle, levels, two_blobs):
    blob = two_blobs[0]
    proofs, evals = levels(blob, 6)
    cells, want = oracle.compute_cells_and_kzg_proofs(blob)
    assert (cells, want) == hip.compute_cells_and_kzg_proofs(blob)
    assert proofs == want and evals == b"".join(cells)
    c = hip.blob_to_kzg_commitment(blob)
    got_cells = [evals[2048 * i:2048 * i + 2048] for i in range(128)]
    assert hip.verify_cell_kzg_proof_batch([c] * 128, list(range(128)), got_cells, proofs)
    assert oracle.verify_cell_kzg_proof_batch([c] * 128, list(range(128)), got_cells, proofs)


@pytest.mark.parametrize("e", range(1, 7))
def test_every_size_hangs_on_the_one_below(levels, g1, two_blobs, e):
    """all relations of the level: 8192 >> e of them"""
    blob = two_blobs[0]
    lower, ev_lo = levels(blob, e - 1)
    got, ev = levels(blob, e)
    assert ev == ev_lo                       # the same bytes for every e
    assert got == _ladder(g1, lower, e)


@pytest.mark.parametrize("e", range(1, 4))
def test_the_second_blob_down_to_size_8(hip, levels, g1, two_blobs, e):
    """the batch tests below compare with this blob's proofs at size 8: they hang on size one, all relations"""
    blob = two_blobs[1]
    lower = levels(blob, e - 1)[0]
    if e == 1:
        assert lower == hip.compute_domain_kzg_proofs_batch([blob])[0][0] + hip.compute_kzg_proof_batch([blob] * 4096, EXT[4096:])[0]
    assert levels(blob, e)[0] == _ladder(g1, lower, e)
    assert levels(blob, e)[1] == b"".join(hip.compute_cells_and_kzg_proofs(blob)[0])


def test_size_8_by_definition(hip, g1):
    """a polynomial of degree 23: q_c has 16 coefficients, q_i = p[i + 8] + a q_{i + 8}, a = x_c^8; the proof is
    sum q_i g1_values_monomial[i] on the setup file's points"""
    lines = open(TRUSTED_SETUP).read().split()
    assert (int(lines[0]), int(lines[1])) == (4096, 65)
    mono = [_jac(g1, bytes.fromhex(h)) for h in lines[2 + 4096 + 65:2 + 4096 + 65 + 16]]
    assert _compress(g1, mono[0]) == G48
    rnd = random.Random(23)
    p = [rnd.randrange(R) for _ in range(24)]
    proofs, st = hip.compute_coset_kzg_proofs_batch([D.blob_of_poly(p)], 3)
    assert st == [0]
    for c in [0, 1, 2, 511, 512, 700, 1022, 1023]:
        q = E.quotient(p, 8, pow(ZS[8 * c], 8, R))
        assert len(q) == 16
        acc = g1.inf
        for qi, pt in zip(q, mono):
            acc = g1.add(acc, g1.mul(pt, qi))
        assert proofs[0][c] == _compress(g1, acc), c


# ---- edge polynomials ----

@pytest.mark.parametrize("e", [0, 3, 6])
def test_edge_polynomials(hip, levels, g1, e):
    l, m = 1 << e, _m(e)
    rnd = random.Random(90 + e)
    zero, const = D.blob_of_poly([]), D.blob_of_poly([0x1234567])
    below = D.blob_of_poly([rnd.randrange(R) for _ in range(l)])               # degree l - 1: the quotient is zero
    xl = D.blob_of_poly([0] * l + [1])                                         # X^l: the quotient is one
    top = D.blob_of_poly([0] * 4095 + [1])
    full = D.blob_of_poly([rnd.randrange(R) for _ in range(4095)] + [R - 1])
    proofs, st = hip.compute_coset_kzg_proofs_batch([zero, const, below, xl, top, full], e)
    assert st == [0] * 6
    assert proofs[0] == [INF48] * m and proofs[1] == [INF48] * m and proofs[2] == [INF48] * m
    assert proofs[3] == [G48] * m
    for i, blob in ((4, top), (5, full)):
        if e == 0:
            inner, st = hip.compute_domain_kzg_proofs_batch([blob])
            outer, _, st2 = hip.compute_kzg_proof_batch([blob] * 4096, EXT[4096:])
            assert st == [0] and st2 == [0] * 4096
            assert proofs[i] == inner[0] + outer
        elif e == 6:
            assert proofs[i] == hip.compute_cells_and_kzg_proofs(blob)[1]
        else:   # down the ladder to size one from the anchors: the first and the last coset and 126 sampled ones
            size_one = hip.compute_domain_kzg_proofs_batch([blob])[0][0] + hip.compute_kzg_proof_batch([blob] * 4096, EXT[4096:])[0]
            for c in [0, m - 1] + random.Random(i).sample(range(1, m - 1), 126):
                assert proofs[i][c] == _ladder_at(g1, size_one, e, c), c


# ---- batches ----

def _raw():
    f = C.CDLL(HIP_SO).ckzg_hip_compute_coset_kzg_proofs_batch
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    return f


def test_a_bad_blob_in_a_batch(hip, levels, two_blobs):
    e, per = 3, _m(3) * 48
    want = [b"".join(levels(b, e)[0]) for b in two_blobs]
    bad = two_blobs[0][:32 * 77] + R.to_bytes(32, "big") + two_blobs[0][32 * 78:]
    proofs, evals, st = hip.compute_coset_kzg_proofs_batch([two_blobs[0], bad, two_blobs[1]], e, want_evals=True)
    assert st == [0, 1, 0]
    assert b"".join(proofs[0]) == want[0] and b"".join(proofs[2]) == want[1]
    assert evals[0] == levels(two_blobs[0], e)[1] and evals[2] == levels(two_blobs[1], e)[1]
    f = _raw()
    out = C.create_string_buffer(3 * per)
    assert f(out, None, None, two_blobs[0] + bad + two_blobs[1], 3, e, hip.sp) == BADARGS   # status and evals may be NULL
    assert out.raw[:per] == want[0] and out.raw[2 * per:] == want[1]
    assert f(out, None, None, bad, 1, e, hip.sp) == BADARGS
    # n = 0, NULL arguments, a coset size the library does not serve: nothing is written
    assert f(None, None, None, None, 0, e, hip.sp) == 0
    assert hip.compute_coset_kzg_proofs_batch([], e) == ([], [])
    assert hip.compute_coset_kzg_proofs_batch([], e, want_evals=True) == ([], [], [])
    keep = out.raw
    st1 = (C.c_uint8 * 1)(7)
    assert f(None, None, st1, two_blobs[0], 1, e, hip.sp) == BADARGS
    assert f(out, None, st1, None, 1, e, hip.sp) == BADARGS
    assert f(out, None, st1, two_blobs[0], 1, 7, hip.sp) == BADARGS
    assert f(None, None, None, None, 0, 7, hip.sp) == BADARGS
    assert out.raw == keep and st1[0] == 7


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_chunk_edge(hip, levels, two_blobs, n):
    e = 3
    rnd = random.Random(n)
    pick = [rnd.randrange(2) for _ in range(n)]
    pick[0], pick[n - 1] = 0, 1
    if n > CHUNK:
        pick[CHUNK - 1], pick[CHUNK] = 1, 0
    proofs, evals, st = hip.compute_coset_kzg_proofs_batch([two_blobs[i] for i in pick], e, want_evals=True)
    assert st == [0] * n
    for i in range(n):
        assert (proofs[i], evals[i]) == levels(two_blobs[pick[i]], e), i


# ---- the device form ----

def _device_call(hip, rt, blobs, e, host_status=False, want_evals=True):
    n = len(blobs)
    sizes = [_m(e) * 48 * n, 8192 * 32 * n, n, BLOB * n]
    ptrs = []
    try:
        for sz in sizes:
            p = C.c_void_p()
            assert rt.hipMalloc(C.byref(p), max(sz, 1)) == 0
            ptrs.append(p)
        data = b"".join(blobs)
        assert rt.hipMemcpy(ptrs[3], C.c_char_p(data), len(data), 1) == 0
        assert rt.hipMemcpy(ptrs[2], C.c_char_p(b"\x07" * n), n, 1) == 0   # (every status byte is written)
        f = hip.lib.ckzg_hip_compute_coset_kzg_proofs_batch_device
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        if host_status:
            return f(ptrs[0], ptrs[1], C.cast((C.c_uint8 * n)(), C.c_void_p), ptrs[3], n, e, hip.sp)
        ret = f(ptrs[0], ptrs[1] if want_evals else None, ptrs[2], ptrs[3], n, e, hip.sp)
        out, ev, st = C.create_string_buffer(sizes[0]), C.create_string_buffer(sizes[1]), C.create_string_buffer(n)
        assert rt.hipMemcpy(out, ptrs[0], sizes[0], 2) == 0 and rt.hipMemcpy(ev, ptrs[1], sizes[1], 2) == 0
        assert rt.hipMemcpy(st, ptrs[2], n, 2) == 0
        return ret, out.raw, ev.raw, list(st.raw)
    finally:
        for p in ptrs:
            rt.hipFree(p)


def test_device_form(hip, rt, levels, two_blobs):  # noqa: F811
    e, per, per_ev = 3, _m(3) * 48, 8192 * 32
    bad = two_blobs[1][:-32] + b"\xff" * 32
    blobs = [two_blobs[1], bad, two_blobs[0]]
    hp, hev, hs = hip.compute_coset_kzg_proofs_batch(blobs, e, want_evals=True)
    ret, out, ev, st = _device_call(hip, rt, blobs, e)
    assert ret == 0 and st == hs == [0, 1, 0]   # invalid blobs are reported through d_status only
    assert out[:per] == b"".join(hp[0]) == b"".join(levels(two_blobs[1], e)[0])
    assert out[2 * per:] == b"".join(hp[2]) == b"".join(levels(two_blobs[0], e)[0])
    assert ev[:per_ev] == hev[0] == levels(two_blobs[1], e)[1] and ev[2 * per_ev:] == hev[2]
    ret, out2, _, st = _device_call(hip, rt, blobs, e, want_evals=False)   # d_evals may be NULL
    assert ret == 0 and st == [0, 1, 0] and out2[:per] == out[:per] and out2[2 * per:] == out[2 * per:]
    assert _device_call(hip, rt, blobs[:1], e, host_status=True) == BADARGS   # a host pointer: nothing launched
    f = hip.lib.ckzg_hip_compute_coset_kzg_proofs_batch_device
    assert f(None, None, None, None, 0, e, hip.sp) == 0
    assert f(None, None, None, None, 1, e, hip.sp) == BADARGS
    assert f(None, None, None, None, 0, 7, hip.sp) == BADARGS


# ---- the lazy setup ----

def test_lazy_setup_of_two_sizes(levels, two_blobs):
    """a size's transformed setup is built by the first call with it on fresh settings and does not disturb another's;
    the tables' bytes are those of the load"""
    def table_bytes(k):
        f = k.lib.ckzg_hip_table_bytes
        f.restype = C.c_uint64
        return f(k.sp)

    opts = {"commit_wbits": 8, "proof_wbits": 6}
    api = Kzg(HIP_SO, "", precompute=0, options=opts)
    try:
        before = table_bytes(api)
        assert before > 0
        blob = two_blobs[1]
        first = api.compute_coset_kzg_proofs_batch([blob], 4, want_evals=True)
        assert first == ([levels(blob, 4)[0]], [levels(blob, 4)[1]], [0])
        assert api.compute_coset_kzg_proofs_batch([blob], 1)[0][0] == levels(blob, 1)[0]
        assert api.compute_coset_kzg_proofs_batch([blob], 4, want_evals=True) == first
        assert api.compute_coset_kzg_proofs_batch([blob], 0)[0][0][:4096] == api.compute_domain_kzg_proofs_batch([blob])[0][0]
        assert table_bytes(api) == before
    finally:
        api.close()
        for k, v in ((b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


# ---- one pipeline behind the domain call and the coset call ----

def _on_fresh_settings(calls):
    """the results of `calls` in turn on settings of their own, which have built no transformed setup yet"""
    api = Kzg(HIP_SO, "", precompute=0, options={"commit_wbits": 8, "proof_wbits": 6})
    try:
        return [call(api) for call in calls]
    finally:
        api.close()
        for k, v in ((b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


def test_the_domain_call_and_size_one_share_their_setup_in_either_order(oracle, levels, two_blobs):
    """both calls read the transformed setup of coset size one, whichever of them built it, and one scratch layout at
    4096 and at 8192 proofs per blob"""
    blob = two_blobs[0]
    want, evals = levels(blob, 0)          # (pinned above to the per-point call and the CPU oracle)
    domain = lambda api: api.compute_domain_kzg_proofs_batch([blob])
    size_one = lambda api: api.compute_coset_kzg_proofs_batch([blob], 0, want_evals=True)
    for calls in ([domain, size_one, domain], [size_one, domain, size_one]):
        for call, got in zip(calls, _on_fresh_settings(calls)):
            assert got == (([want[:4096]], [0]) if call is domain else ([want], [evals], [0]))
    for j in (0, 4095) + tuple(random.Random(12).sample(range(1, 4095), 3)):
        assert oracle.compute_kzg_proof(blob, EXT[j])[0] == want[j], j


def test_the_domain_call_ignores_what_a_coset_call_left_in_the_rows(levels, two_blobs):
    """size 8 works on the first 1024 entries of a row and leaves the products of its columns above them; the domain
    call's last transform of 4096 reads none of the upper half, which it does not clear"""
    blob = two_blobs[0]
    size_8 = lambda api: api.compute_coset_kzg_proofs_batch([blob], 3, want_evals=True)
    domain = lambda api: api.compute_domain_kzg_proofs_batch([blob])
    got_8, got = _on_fresh_settings([size_8, domain])
    assert got_8 == ([levels(blob, 3)[0]], [levels(blob, 3)[1]], [0])
    assert got == ([levels(blob, 0)[0][:4096]], [0])
