"""G1 validation on every GPU path that decides it, against the corpus of tests/g1_points.py (valid points, points
outside G1 of every torsion order, bad encodings; pinned on the CPU by tests/test_g1_corpus.py).  A batch verifier
is sound only if it answers C_KZG_BADARGS for every commitment or proof that is not a point of G1
(src/common/bytes.c:81-95); the library decides that in four places, picked by batch size, options and where the
inputs live:

  * k_validate_g1<1> + k_subgroup_g1_quad (verify.hip): host-pointer blob batches of 4..1023, cell batches;
  * k_subgroup_g1, one lane per point: more than 32768 points (ckzg_hip_g1_lincomb, large cell batches);
  * k_validate_g1<0>, decompression and subgroup test fused: host batches >= 1024, every resident batch;
  * the host test of batches of <= 3 blobs.

Expected outcomes come from the corpus and the CPU oracle, never from the library.  Then one row per form of
verify_blobs_core (ckzg_api2.hip) and of the cell verification: a valid batch, a wrong proof, a commitment and a proof
outside G1, a non-canonical field element, at the first and the last blob."""
import ctypes as C

import pytest

import g1_points as GP
from conftest import ORACLE_SO
from test_gpu_commitment import R, rand_blob

pytestmark = pytest.mark.gpu

CORPUS = GP.corpus()
INF48 = bytes([0xc0]) + bytes(47)
BLOB = 131072
# option defaults (ckzg_api.hip): restored after every test that changes one
DEFAULTS = {"gpu_sha_min": 0, "verify_pipe_min": 1024, "verify_call_table": 1, "verify_cu_partition": 1}


class Options:
    """call-time options set for the body of a with-block, the defaults back on every exit path"""

    def __init__(self, hip, **opts):
        self.hip, self.opts = hip, opts

    def __enter__(self):
        for k, v in self.opts.items():
            assert self.hip.lib.ckzg_hip_set_option(k.encode(), v) == 0, k

    def __exit__(self, *exc):
        for k in self.opts:
            self.hip.lib.ckzg_hip_set_option(k.encode(), DEFAULTS[k])


@pytest.fixture(scope="module")
def rt():
    lib = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    lib.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    lib.hipHostFree.argtypes = [C.c_void_p]
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.hipFree.argtypes = [C.c_void_p]
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return lib


@pytest.fixture(scope="module")
def material(oracle):
    """eight blobs with the oracle's commitments and proofs, and the zero blob (commitment and proof: infinity)"""
    blobs = [rand_blob(0x61, i) for i in range(8)]
    cm = [oracle.blob_to_kzg_commitment(b) for b in blobs]
    pr = [oracle.compute_blob_kzg_proof(b, c) for b, c in zip(blobs, cm)]
    zero = bytes(BLOB)
    assert oracle.blob_to_kzg_commitment(zero) == INF48 and oracle.compute_blob_kzg_proof(zero, INF48) == INF48
    return blobs, cm, pr


def _order(n):
    return [(3 * i + i // 11) % 8 for i in range(n)]


def _as_ptr(x):
    if isinstance(x, C.c_void_p):
        return x
    if isinstance(x, bytearray):
        return C.cast((C.c_char * len(x)).from_buffer(x), C.c_void_p)
    return C.cast(C.c_char_p(x), C.c_void_p)


def _verify_host(hip, bb, cc, pp, n):
    f = hip.lib.verify_blob_kzg_proof_batch
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p]
    ok = C.c_bool(False)
    rc = f(C.byref(ok), _as_ptr(bb), _as_ptr(cc), _as_ptr(pp), n, C.addressof(hip.s))
    return rc, ok.value


class Batch:
    """n blobs with commitments and proofs in one of three homes -- pageable host memory, page-locked host memory, HBM
    (the resident entry point) -- whose blob bytes, commitments and proofs can be patched in place and put back."""

    def __init__(self, hip, rt, material, n, home):
        blobs, cm, pr = material
        self.hip, self.rt, self.n, self.home = hip, rt, n, home
        self.order = _order(n)
        self.cc = b"".join(cm[k] for k in self.order)
        self.pp = b"".join(pr[k] for k in self.order)
        self.bb = bytearray(b"".join(blobs[k] for k in self.order))
        self.buf = None
        if home == "pinned":
            self.buf = C.c_void_p()
            assert rt.hipHostMalloc(C.byref(self.buf), len(self.bb), 0) == 0
            C.memmove(self.buf, _as_ptr(self.bb), len(self.bb))
        elif home == "device":
            self.dev = [C.c_void_p() for _ in range(3)]
            for q, size in zip(self.dev, (len(self.bb), 48 * n, 48 * n)):
                assert rt.hipMalloc(C.byref(q), max(size, 1)) == 0
            assert rt.hipMemcpy(self.dev[0], _as_ptr(self.bb), len(self.bb), 1) == 0

    def close(self):
        if self.home == "pinned":
            self.rt.hipHostFree(self.buf)
        elif self.home == "device":
            for q in self.dev:
                self.rt.hipFree(q)

    def _put_blob_bytes(self, off, data):
        self.bb[off:off + len(data)] = data
        if self.home == "pinned":
            C.memmove(self.buf.value + off, data, len(data))
        elif self.home == "device":
            assert self.rt.hipMemcpy(C.c_void_p(self.dev[0].value + off), C.c_char_p(data), len(data), 1) == 0

    def verify(self, cc=None, pp=None, spoil=None):
        """(C_KZG_RET, verdict); spoil = blob index whose element 1234 is made r (non-canonical) for this call"""
        cc, pp = cc or self.cc, pp or self.pp
        if spoil is not None:
            off = spoil * BLOB + 32 * 1234
            keep = bytes(self.bb[off:off + 32])
            self._put_blob_bytes(off, R.to_bytes(32, "big"))
        try:
            if self.home == "device":
                assert self.rt.hipMemcpy(self.dev[1], C.c_char_p(cc), len(cc), 1) == 0
                assert self.rt.hipMemcpy(self.dev[2], C.c_char_p(pp), len(pp), 1) == 0
                f = self.hip.lib.ckzg_hip_verify_blob_kzg_proof_batch_device
                f.restype = C.c_int
                f.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p]
                ok = C.c_bool(False)
                rc = f(C.byref(ok), self.dev[0], self.dev[1], self.dev[2], self.n, C.addressof(self.hip.s))
                return rc, ok.value
            return _verify_host(self.hip, self.buf if self.home == "pinned" else self.bb, cc, pp, self.n)
        finally:
            if spoil is not None:
                self._put_blob_bytes(off, keep)


def _put(seq, i, item):
    return seq[:48 * i] + item + seq[48 * (i + 1):]


# ---------------------------------------------------------------------------------------------------------------------
# k_validate_g1<1> + k_subgroup_g1_quad: host-pointer batch of 9 blobs, 18 points -- a full workgroup of 16 points and a
# ragged one whose dead lanes repeat the last point.  Status index s: commitment s (s < n), proof s - n.
# ---------------------------------------------------------------------------------------------------------------------

N9 = 9


@pytest.mark.parametrize("s", [0, 15, 16, N9 - 1, N9, 2 * N9 - 1])
def test_split_validation_kernels_on_the_corpus(hip, oracle, material, s):
    blobs, cm, pr = material
    order = _order(N9)
    with Options(hip, gpu_sha_min=1 << 20):   # host hash: the split form of a small host-pointer batch
        for e in CORPUS:
            bl = [blobs[k] for k in order]
            cs = [cm[k] for k in order]
            ps = [pr[k] for k in order]
            i = s % N9
            if e.point is GP.INF:
                bl[i], cs[i], ps[i] = bytes(BLOB), INF48, INF48   # infinity with the zero blob: a true batch
            (cs if s < N9 else ps)[i] = e.data
            rc, ok = _verify_host(hip, b"".join(bl), b"".join(cs), b"".join(ps), N9)
            if e.expected != GP.VALID:
                assert rc == 1, (e.label, s, rc, ok)
                continue
            want = oracle.verify_blob_kzg_proof_batch(bl, cs, ps)
            if e.point is GP.INF:
                assert want is True
            assert (rc, ok) == (0, want), (e.label, s, rc, ok, want)


# ---------------------------------------------------------------------------------------------------------------------
# k_subgroup_g1 (one lane per point, > 32768 points) and k_subgroup_g1_quad (<= 32768) through ckzg_hip_g1_lincomb,
# whose subgroup check runs before any sum.  Points go in as g1_t, decoded by the oracle (curve check only).
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def g1_of():
    o = C.CDLL(ORACLE_SO)
    out = {}
    for e in CORPUS:
        if e.expected == GP.BAD_ENCODING:
            continue
        aff, jac = C.create_string_buffer(96), C.create_string_buffer(144)
        assert o.og1_uncompress(aff, e.data) == 0, e.label
        o.og1_from_affine(jac, aff)
        out[e.label] = jac.raw
    return out


@pytest.mark.parametrize("n", [32769, 32768])
def test_subgroup_kernels_of_g1_lincomb_on_the_corpus(hip, g1_of, n):
    f = hip.lib.ckzg_hip_g1_lincomb
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_void_p]
    # filler: the identity (no host inversion per point), with the generator every 1024th point
    gen, inf = g1_of["G"], g1_of["inf"]
    pts = bytearray(b"".join(gen if i % 1024 == 1 else inf for i in range(n)))
    scalars = bytes(32 * n)
    out = C.create_string_buffer(144)
    for at in sorted({0, 32767, n - 1}):
        keep = bytes(pts[144 * at:144 * (at + 1)])
        for e in CORPUS:
            if e.expected == GP.BAD_ENCODING:
                continue
            pts[144 * at:144 * (at + 1)] = g1_of[e.label]
            rc = f(out, _as_ptr(pts), scalars, n, 0, C.addressof(hip.s))
            assert rc == (1 if e.expected == GP.NOT_IN_G1 else 0), (e.label, n, at, rc)
        pts[144 * at:144 * (at + 1)] = keep


# ---------------------------------------------------------------------------------------------------------------------
# k_validate_g1<0> (decompression + subgroup test fused): resident batch of 1030 blobs, 2060 points (a ragged last wave)
# ---------------------------------------------------------------------------------------------------------------------

FUSED_SUBSET = ["T11_0", "T10177_0", "T859267_0", "T52437899_0", "Q+T11", "T3", "neg(T3)", "generic", "x=p",
                "off_curve", "Q"]


def test_fused_validation_kernel_on_the_corpus(hip, rt, material):
    n = 1030
    b = Batch(hip, rt, material, n, "device")
    try:
        assert b.verify() == (0, True)
        for label in FUSED_SUBSET:
            e = GP.by_label(label)
            for s in (0, n - 1, n, 2 * n - 1):
                cc = _put(b.cc, s, e.data) if s < n else b.cc
                pp = _put(b.pp, s - n, e.data) if s >= n else b.pp
                got = b.verify(cc, pp)
                want = (0, False) if e.expected == GP.VALID else (1, False)
                assert got == want, (label, s, got)
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# The forms of verify_blobs_core.  Each row: a valid batch is true; one wrong (valid) proof is false; a commitment
# outside G1, a proof outside G1, a non-canonical field element are BADARGS -- at the first and the last blob (the
# pipelined form: also at the chunk boundary 255 / 256).  Points outside G1 alternate between Q + T11 and T3.
# ---------------------------------------------------------------------------------------------------------------------

BIG = 1 << 20
FORMS = [
    # (id, n, home, options)
    ("small_2", 2, "host", {}),
    ("small_3", 3, "host", {}),
    ("split_ladders_5", 5, "host", {"gpu_sha_min": BIG}),
    ("split_table_host_hash_100", 100, "host", {"gpu_sha_min": BIG}),
    ("split_gpu_hash_300", 300, "host", {"gpu_sha_min": 1}),
    ("split_gpu_hash_partitioned_768", 768, "host", {"gpu_sha_min": 1, "verify_cu_partition": 1}),
    ("whole_host_hash_1030", 1030, "host", {"verify_pipe_min": BIG, "gpu_sha_min": BIG}),
    ("piped_pageable_1030", 1030, "host", {"gpu_sha_min": BIG}),
    ("piped_pinned_1030", 1030, "pinned", {"gpu_sha_min": BIG}),
    ("whole_gpu_hash_partitioned_1030", 1030, "host", {"gpu_sha_min": 1, "verify_cu_partition": 1}),
    ("whole_gpu_hash_1030", 1030, "host", {"gpu_sha_min": 1, "verify_cu_partition": 0}),
    ("resident_partitioned_700", 700, "device", {"verify_cu_partition": 1}),
    ("resident_700", 700, "device", {"verify_cu_partition": 0}),
    ("resident_300", 300, "device", {}),
    ("ladders_split_100", 100, "host", {"gpu_sha_min": BIG, "verify_call_table": 0}),
    ("ladders_split_gpu_hash_partitioned_768", 768, "host",
     {"gpu_sha_min": 1, "verify_cu_partition": 1, "verify_call_table": 0}),
    ("ladders_piped_1030", 1030, "host", {"gpu_sha_min": BIG, "verify_call_table": 0}),
    ("ladders_resident_700", 700, "device", {"verify_call_table": 0}),
]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_verification_forms_reject_what_is_not_in_g1(hip, rt, material, form):
    name, n, home, opts = form
    blobs, cm, pr = material
    non_g1 = [GP.by_label("Q+T11").data, GP.by_label("T3").data]
    assert all(GP.classify(x) == GP.NOT_IN_G1 for x in non_g1)
    positions = [0, n - 1] + ([255, 256] if name.startswith(("piped", "ladders_piped")) else [])
    b = Batch(hip, rt, material, n, home)
    try:
        with Options(hip, **opts):
            assert b.verify() == (0, True), name
            k = 0
            for at in positions:
                wrong = pr[(b.order[at] + 1) % 8]
                assert b.verify(pp=_put(b.pp, at, wrong)) == (0, False), (name, at)
                assert b.verify(cc=_put(b.cc, at, non_g1[k % 2]))[0] == 1, (name, at, "commitment")
                assert b.verify(pp=_put(b.pp, at, non_g1[(k + 1) % 2]))[0] == 1, (name, at, "proof")
                k += 1
                assert b.verify(spoil=at)[0] == 1, (name, at, "field element")
            assert b.verify() == (0, True), name   # every patch was put back
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# verify_cell_kzg_proof_batch: proofs [0, n) and distinct commitments [n, n + nc) through k_validate_g1<1> and the
# subgroup kernel on the second stream -- the quad form up to 32768 points, the one-lane form beyond (n = 32768 cells:
# n + nc > 32768), the flags checked underneath the transcript hash (table) or after the sums (ladders).
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cell_material(oracle, material):
    blobs, cm, _ = material
    return [(cm[j],) + tuple(oracle.compute_cells_and_kzg_proofs(blobs[j])) for j in range(4)]


@pytest.mark.parametrize("n", [100, 300, 32768])
def test_cell_verification_rejects_what_is_not_in_g1(hip, cell_material, n):
    picks = [((7 * i + i // 128) % 4, (5 * i + 3) % 128) for i in range(n)]
    cms = [cell_material[j][0] for j, _ in picks]
    idx = [c for _, c in picks]
    cells = [cell_material[j][1][c] for j, c in picks]
    prs = [cell_material[j][2][c] for j, c in picks]
    assert hip.verify_cell_kzg_proof_batch(cms, idx, cells, prs) is True
    from kzg_ctypes import KzgError
    for k, at in enumerate((0, n - 1)):
        p_bad, c_bad = GP.by_label("Q+T11" if k else "T3").data, GP.by_label("T3" if k else "Q+T11").data
        with pytest.raises(KzgError, match="C_KZG_RET 1"):
            hip.verify_cell_kzg_proof_batch(cms, idx, cells, prs[:at] + [p_bad] + prs[at + 1:])
        with pytest.raises(KzgError, match="C_KZG_RET 1"):
            hip.verify_cell_kzg_proof_batch(cms[:at] + [c_bad] + cms[at + 1:], idx, cells, prs)
    wrong = prs[:n - 1] + [prs[0] if prs[0] != prs[n - 1] else prs[1]]
    assert hip.verify_cell_kzg_proof_batch(cms, idx, cells, wrong) is False
