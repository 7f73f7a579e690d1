"""One family of poison probes in a process of its own (tests/test_gpu_poison.py starts it under tests/watchdog.py):

    python tests/poison/driver.py FAMILY EXPECTED.pickle REPORT.json [FILLS]

(FILLS: the fill bytes of the runs, "0,255,1" unless given; "0,0,0" is how a family's time limit was measured.)

Every probe of the family runs three times in a row on settings loaded for that run -- option "poison_temporaries" off,
0xFF, 0x01 -- into host buffers pre-filled with 0xA5, and what comes back is compared bytewise with EXPECTED, which the
CPU oracle and the Python references made (tests/poison/corpus.py and expected() below; never this library).  The
report is rewritten after every probe, so a child that dies leaves the record up to there.  The child stops at the
first C return it did not expect or the first HIP error, starts nothing further on the GPU, and says which probe it
was in.  No retries.

PROBES is also read without a GPU: the CPU test holds it against c-kzg-4844_amd/exports.map."""
import ctypes as C
import json
import os
import pickle
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import corpus as K  # noqa: E402
import domain_expect as D  # noqa: E402

R = K.R
GUARD = 64
A5 = 0xA5
SMALL_TABLES = {"commit_wbits": 8, "proof_wbits": 6, "fk20_wbits": 8}
DEFAULTS = {"commit_wbits": 10, "proof_wbits": 8, "fk20_wbits": 0, "direct_max": -1, "gpu_sha_min": 0,
            "verify_pipe_min": 1024, "verify_call_table": 1, "locate_max_checks": 1024, "commit_graph": 1,
            "poison_temporaries": 0}
POISONS = (0, 0xFF, 0x01)
U64, U32, INT = C.c_uint64, C.c_uint32, C.c_int


class Stop(Exception):
    """the child ends here: an unexpected return value or a HIP error"""


# ---------------------------------------------------------------------------------------------------------------------
# expected values: oracle, references, golden files.  No GPU.
# ---------------------------------------------------------------------------------------------------------------------

class Source:
    """what the oracle says about the corpus blobs, each asked once"""

    def __init__(self, orc=None):
        self.o = orc or K.load_oracle()
        self.m = {}

    def _memo(self, key, make):
        if key not in self.m:
            self.m[key] = make()
        return self.m[key]

    def blob(self, i):
        return self._memo(("blob", i), lambda: K.blob(i))

    def cm(self, i):
        return self._memo(("cm", i), lambda: self.o.blob_to_kzg_commitment(self.blob(i)))

    def bproof(self, i):
        return self._memo(("bproof", i), lambda: self.o.compute_blob_kzg_proof(self.blob(i), self.cm(i)))

    def kzg(self, i, z):
        return self._memo(("kzg", i, z), lambda: self.o.compute_kzg_proof(self.blob(i), z))

    def cells(self, i):
        return self._memo(("cells", i), lambda: self.o.compute_cells_and_kzg_proofs(self.blob(i)))


def _base(src, nblobs=3):
    return {"blobs": [src.blob(i) for i in range(nblobs)], "bad": K.non_canonical(src.blob(1)),
            "cm": [src.cm(i) for i in range(nblobs)]}


def _coset_proofs(src, b, e):
    return {0: lambda: K.golden(b)[0], 3: lambda: K.golden(b)[1], 6: lambda: src.cells(b)[1]}[e]()


def _coset_item(src, b, e, c):
    """(commitment, coset index, values, proof) of coset c of blob b at coset size 2^e: true by construction"""
    ev = b"".join(src.cells(b)[0])
    w = 32 << e
    return (src.cm(b), c, ev[c * w:(c + 1) * w], _coset_proofs(src, b, e)[c])


def _spoil_value(item):
    cm, c, ev, pr = item
    return (cm, c, K.bump(ev[:32]) + ev[32:], pr)


def _bad_value(item):
    cm, c, ev, pr = item
    return (cm, c, ev[:-32] + R.to_bytes(32, "big"), pr)


def expected_commit(src):
    return _base(src)


def expected_proofs(src):
    d = _base(src)
    z_in, z_in2, z_off = K.EXT[5], K.EXT[4000], K.fr(0x1234567)
    d.update(z_in=z_in, z_off=z_off, z_bad=R.to_bytes(32, "big"),
             kzg_in=src.kzg(0, z_in), kzg_off=src.kzg(0, z_off), kzg_in2=src.kzg(2, z_in2), z_in2=z_in2,
             bproof=[src.bproof(i) for i in range(3)], evals0=b"".join(src.cells(0)[0]),
             coset={e: b"".join(_coset_proofs(src, 0, e)) for e in (0, 3, 6)})
    return d


def expected_cells(src):
    d = _base(src, 2)
    d.update(cells=[b"".join(src.cells(i)[0]) for i in range(2)], cproofs=[b"".join(src.cells(i)[1]) for i in range(2)])
    return d


def expected_recover(src):
    d = expected_cells(src)
    d["coset"] = {e: [b"".join(_coset_proofs(src, b, e)) for b in range(2)] for e in (0, 3, 6)}
    return d


def _point_items(src):
    """(commitment, z, y, proof, verdict, status): true ones from the oracle's proofs, then spoilt in one place"""
    z_in, z_off = K.EXT[5], K.fr(0x1234567)
    p_in, y_in = src.kzg(0, z_in)
    p_off, y_off = src.kzg(0, z_off)
    p2, y2 = src.kzg(2, K.EXT[4000])
    good = (src.cm(0), z_off, y_off, p_off, True, 0)
    items = [good,
             (src.cm(0), z_off, K.bump(y_off), p_off, False, 0),          # one bumped value
             (b"\xff" * 48, z_off, y_off, p_off, False, 1),                # an invalid encoding
             (src.cm(0), z_in, y_in, p_in, True, 0),                       # z on the domain
             (src.cm(2), K.EXT[4000], y2, p_off, False, 0)]                # a swapped proof
    from kzg_ctypes import KzgError
    for cm, z, y, p, ok, st in items:   # the oracle agrees with the construction
        try:
            verdict, refused = src.o.verify_kzg_proof(cm, z, y, p), None
        except KzgError as e:           # (the oracle's binding raises for a return value that is not C_KZG_OK)
            verdict, refused = None, str(e)
        if st == 0:
            assert refused is None and verdict is ok, (refused, verdict, ok)
        else:
            assert refused is not None and "C_KZG_RET 1" in refused, refused
    return items


def expected_verify(src):
    d = _base(src)
    d.update(bproof=[src.bproof(i) for i in range(3)], items=_point_items(src),
             challenge=src.o.compute_challenge(src.blob(0), src.cm(0)))
    return d


def _cell_items(src):
    c0, p0 = src.cells(0)
    c1, p1 = src.cells(1)
    return [(src.cm(0), 3, c0[3], p0[3]), (src.cm(1), 127, c1[127], p1[127]), (src.cm(0), 64, c0[64], p0[64]),
            (src.cm(1), 0, c1[0], p1[0]), (src.cm(0), 3, c0[3], p0[3])]


def expected_cell_verify(src):
    d = {"cells3": _cell_items(src)[:3]}
    c0, p0 = src.cells(0)
    c1, p1 = src.cells(1)
    # the smallest batch that builds the call-time table: 128 cells of two blobs, cell 5 of blob 0 twice
    many = [(src.cm(0), i, c0[i], p0[i]) for i in range(100)] + [(src.cm(1), i, c1[i], p1[i]) for i in range(27)]
    many.insert(64, many[5])
    assert len(many) == 128 and src.o.verify_cell_kzg_proof_batch(*[list(t) for t in zip(*many)])
    d["cells128"] = many
    d["locate"] = _cell_items(src)
    d["coset"] = {e: [_coset_item(src, 0, e, 1), _coset_item(src, 1, e, (8192 >> e) - 1), _coset_item(src, 0, e, 70),
                      _coset_item(src, 1, e, 2)] for e in (0, 3, 6)}
    cms, idx, cells, proofs = [list(t) for t in zip(*d["cells3"])]
    d["challenge"] = src.o.compute_verify_cell_kzg_proof_batch_challenge([src.cm(0), src.cm(1)], [0, 1, 0], idx, cells, proofs)
    d["challenge_in"] = ([src.cm(0), src.cm(1)], [0, 1, 0], idx, cells, proofs)
    return d


def expected_groups(src):
    d = _base(src)
    d.update(bproof=[src.bproof(i) for i in range(3)], cell_items=_cell_items(src),
             cproofs=[list(src.cells(i)[1]) for i in range(2)],
             coset={e: [_coset_item(src, 0, e, 1), _coset_item(src, 1, e, (8192 >> e) - 1), _coset_item(src, 0, e, 70),
                        _coset_item(src, 1, e, 2)] for e in (0, 3, 6)})
    return d


def expected_g1(src=None):
    import random
    g1 = K.OracleG1()
    rnd = random.Random(0x901)
    d = {"fft": {}, "prefix": {}}

    def point(a):   # a G with a Z that is not one
        if a == 0:
            return g1.inf
        j = rnd.randrange(1, R)
        return g1.add(g1.mul(g1.gen, (a - j) % R), g1.mul(g1.gen, j))

    for n in (2, 64, 256):
        a = [rnd.randrange(1, R) for _ in range(n)]
        if n >= 4:
            a[1], a[3] = 0, a[2]            # the identity among the inputs, and a repeated point
        w = D.root_of_unity(n)
        d["fft"][n] = {"in": [point(v) for v in a],
                       0: [g1.mul(g1.gen, v) if v else g1.inf for v in D.fft(a, w)],
                       1: [g1.mul(g1.gen, v) if v else g1.inf for v in D.fft(a, pow(w, -1, R))]}
    for n in (1, 300):
        a = [rnd.randrange(1, R) for _ in range(n)]
        if n > 1:
            a[150] = 0                       # an identity in the middle
        acc, sums = 0, []
        for v in a:
            acc = (acc + v) % R
            sums.append(g1.mul(g1.gen, acc) if acc else g1.inf)
        d["prefix"][n] = {"in": [point(v) for v in a], "out": sums}
    n = 130
    a = [rnd.randrange(1, R) for _ in range(n)]
    k = [rnd.randrange(R) for _ in range(n)]
    a[7] = 0                                 # an infinity
    a[21], k[21] = R - a[20], k[20]          # P, -P with one scalar: the pair cancels
    fr = C.create_string_buffer(32)
    mont = []
    for v in k:
        g1.o.ofr_from_raw(fr, (C.c_uint64 * 4)(*[(v >> (64 * i)) & (2 ** 64 - 1) for i in range(4)]))
        mont.append(fr.raw)
    total = sum(x * y for x, y in zip(a, k)) % R
    d["lincomb"] = {"in": [point(v) for v in a], "coeffs": mont, "out": g1.mul(g1.gen, total)}
    return d


# ---------------------------------------------------------------------------------------------------------------------
# the child's tools
# ---------------------------------------------------------------------------------------------------------------------

class Out:
    """a host buffer handed to the library: n bytes and a guard behind them, all 0xA5"""

    def __init__(self, n):
        self.n = n
        self.buf = C.create_string_buffer(bytes([A5]) * (n + GUARD), n + GUARD)

    @property
    def raw(self):
        return self.buf.raw[:self.n]

    def guard_ok(self):
        return self.buf.raw[self.n:] == bytes([A5]) * GUARD


class Run:
    """one run of a family's probes under one fill byte"""

    def __init__(self, rt, data):
        self.rt, self.d, self.fails, self.k, self.k2 = rt, data, [], None, None
        self.stopped = False    # set by stop(): from then on the child makes no call it can do without
        self.notes = {}         # what a probe wants on record beside its failures

    def stop(self, why):
        self.stopped = True
        raise Stop(why)

    def call(self, k, name, *args, allow=(0,)):
        f = getattr(k.lib, name)
        f.restype = C.c_int
        ret = f(*args)
        if ret not in allow:
            self.stop("%s returned %d, expected %s" % (name, ret, list(allow)))
        return ret

    def opt(self, key, value):
        f = self.k.lib.ckzg_hip_set_option
        f.restype, f.argtypes = C.c_int, [C.c_char_p, C.c_int64]
        if f(key.encode(), value) != 0:
            self.stop("option %s = %d refused" % (key, value))

    def eq(self, label, got, want, skip=()):
        """got: bytes or an Out (whose guard is checked too); skip: (lo, hi) byte ranges that are unspecified"""
        if isinstance(got, Out):
            if not got.guard_ok():
                self.fails.append("%s: bytes behind the output were written" % label)
            got = got.raw
        if len(got) != len(want):
            self.fails.append("%s: %d bytes, expected %d" % (label, len(got), len(want)))
            return
        for lo, hi in skip:
            got = got[:lo] + want[lo:hi] + got[hi:]
        if got != want:
            at = next(i for i in range(len(want)) if got[i] != want[i])
            self.fails.append("%s: differs from byte %d of %d (got %s, expected %s)" %
                              (label, at, len(want), got[at:at + 8].hex(), want[at:at + 8].hex()))

    def true(self, label, cond):
        if not cond:
            self.fails.append(label)

    # device memory of the test's own (the *_device forms)
    def dev(self, data):
        p = C.c_void_p()
        if self.rt.hipMalloc(C.byref(p), max(len(data), 1)) != 0 or self.rt.hipMemcpy(p, data, len(data), 1) != 0:
            self.stop("the test's own hipMalloc / hipMemcpy failed")
        return p

    def dev_out(self, n):
        return self.dev(bytes([A5]) * (n + GUARD))

    def back(self, label, p, n):
        """the n bytes at p; the guard behind them is checked"""
        buf = C.create_string_buffer(n + GUARD)
        if self.rt.hipMemcpy(buf, p, n + GUARD, 2) != 0:
            self.stop("the test's own hipMemcpy back failed")
        self.true("%s: bytes behind the device output were written" % label, buf.raw[n:] == bytes([A5]) * GUARD)
        return buf.raw[:n]

    def free(self, *ptrs):
        if self.stopped:        # (the process is about to end: its memory goes with it)
            return
        for p in ptrs:
            self.rt.hipFree(p)


def hip_runtime():
    rt = C.CDLL("libamdhip64.so")
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipFree.argtypes = [C.c_void_p]
    return rt


def statuses(n, bad):
    return bytes(1 if i in bad else 0 for i in range(n))


def skips(per, bad):
    return [(per * i, per * (i + 1)) for i in bad]


# ---------------------------------------------------------------------------------------------------------------------
# commit
# ---------------------------------------------------------------------------------------------------------------------

def p_commit_one(r):
    d, k = r.d, r.k
    for graph, b in ((1, 0), (1, 0), (0, 1), (2, 2)):   # as a graph: built, then launched again; plain; built anew
        r.opt("commit_graph", graph)
        out = Out(48)
        r.call(k, "blob_to_kzg_commitment", out.buf, d["blobs"][b], k.sp)
        r.eq("one blob, commit_graph = %d" % graph, out, d["cm"][b])
    r.opt("commit_graph", 1)
    out = Out(48)
    r.call(k, "blob_to_kzg_commitment", out.buf, d["bad"], k.sp, allow=(1,))
    out = Out(48)
    r.call(k, "blob_to_kzg_commitment", out.buf, d["blobs"][2], k.sp)
    r.eq("one blob after a non-canonical one", out, d["cm"][2])


def _commit_batch(r, label, pick, bad):
    d, k = r.d, r.k
    n = len(pick)
    blobs = b"".join(d["bad"] if i in bad else d["blobs"][pick[i]] for i in range(n))
    out, st = Out(48 * n), Out(n)
    r.call(k, "ckzg_hip_blob_to_kzg_commitment_batch", out.buf, st.buf, blobs, U64(n), k.sp, allow=(1,))
    r.eq(label + ": status", st, statuses(n, bad))
    r.eq(label + ": commitments", out, b"".join(d["cm"][p] for p in pick), skips(48, bad))


def p_commit_batch5(r):
    _commit_batch(r, "5 blobs", [0, 1, 2, 1, 0], {1})


def p_commit_batch65(r):
    # two staging chunks; blob 64, the second chunk's only one, is non-canonical, and so is blob 10 with good ones after
    _commit_batch(r, "65 blobs", [i % 3 for i in range(65)], {10, 64})


def p_commit_batch133(r):
    # The deferred form: chunks of 64 and 69 blobs, both cut into at most 8 partial sums a blob (commit_chunk_fits8), so
    # the sums are parked in d_part8 across the chunks and finalized once; the second chunk writes 7 of a blob's 8
    # places.  (65 blobs do not get there: a chunk of one blob is cut finer.)  A non-canonical blob in either chunk.
    _commit_batch(r, "133 blobs", [(i * 7 + i // 3) % 3 for i in range(133)], {10, 100})


def p_commit_device(r):
    d, k = r.d, r.k
    pick, bad = [0, 1, 2, 1, 0], {1}
    n = len(pick)
    d_blobs = r.dev(b"".join(d["bad"] if i in bad else d["blobs"][pick[i]] for i in range(n)))
    d_out, d_st = r.dev_out(48 * n), r.dev_out(n)
    try:
        r.call(k, "ckzg_hip_blob_to_kzg_commitment_batch_device", d_out, d_st, d_blobs, U64(n), k.sp)
        r.eq("device form: status", r.back("status", d_st, n), statuses(n, bad))
        r.eq("device form: commitments", r.back("commitments", d_out, 48 * n), b"".join(d["cm"][p] for p in pick), skips(48, bad))
    finally:
        r.free(d_blobs, d_out, d_st)


COMBINER_ROUNDS = 20


def _coalesce_stats(k, op=0):
    """ckzg_hip_coalesce_stats of the commitment combiner: calls, solo, batches, batched, ..."""
    f = k.lib.ckzg_hip_coalesce_stats
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_int]
    v = (C.c_uint64 * 9)()
    if f(C.addressof(k.s), op, v, 9) != 9:
        return None
    return dict(zip(("calls", "solo", "batches", "batched"), (int(x) for x in v[:4])))


def p_commit_threads(r):
    """Four callers at once: more than stay on their own, so the combiner's page-locked batch serves some of them.
    Whether a call is batched is a matter of timing, so rounds of four threads x three calls go on until the
    combiner's own count says that a batch has served a call (at most COMBINER_ROUNDS of them; none is a failure).
    A caller that gets a return value other than C_KZG_OK says so at once, and no thread starts another call."""
    d, k = r.d, r.k
    f = k.lib.blob_to_kzg_commitment
    f.restype = C.c_int
    before = _coalesce_stats(k)
    if before is None:
        r.stop("ckzg_hip_coalesce_stats gave no figures: the combiner is off")
    halt = threading.Event()
    rounds, after = 0, before
    while rounds < COMBINER_ROUNDS and after["batched"] == before["batched"]:
        rounds += 1
        res, gate = [[] for _ in range(4)], threading.Barrier(4)

        def caller(t):
            gate.wait()
            for call in range(3):
                if halt.is_set():
                    return
                out = Out(48)
                ret = f(out.buf, d["blobs"][(t + call) % 3], k.sp)
                res[t].append((ret, out))
                if ret != 0:
                    halt.set()
                    return

        th = [threading.Thread(target=caller, args=(t,)) for t in range(4)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        for t in range(4):
            for call, (ret, out) in enumerate(res[t]):
                if ret != 0:
                    r.stop("blob_to_kzg_commitment of thread %d returned %d" % (t, ret))
                r.eq("round %d, thread %d, call %d" % (rounds, t, call), out, d["cm"][(t + call) % 3])
        after = _coalesce_stats(k)
    r.notes["combiner"] = {"rounds": rounds, "batches": after["batches"] - before["batches"],
                           "batched_calls": after["batched"] - before["batched"], "calls": after["calls"] - before["calls"]}
    r.true("no call of %d rounds of four threads was served by a combiner batch" % rounds, after["batched"] > before["batched"])


# ---------------------------------------------------------------------------------------------------------------------
# proofs
# ---------------------------------------------------------------------------------------------------------------------

def p_kzg_proof(r):
    d, k = r.d, r.k
    for label, z, want in (("on the domain", d["z_in"], d["kzg_in"]), ("off the domain", d["z_off"], d["kzg_off"])):
        proof, y = Out(48), Out(32)
        r.call(k, "compute_kzg_proof", proof.buf, y.buf, d["blobs"][0], z, k.sp)
        r.eq("compute_kzg_proof %s: proof" % label, proof, want[0])
        r.eq("compute_kzg_proof %s: y" % label, y, want[1])


def _kzg_batch_io(d):
    blobs = d["blobs"][0] + d["blobs"][1] + d["blobs"][2]
    zs = d["z_off"] + d["z_bad"] + d["z_in2"]
    return blobs, zs, d["kzg_off"][0] + bytes(48) + d["kzg_in2"][0], d["kzg_off"][1] + bytes(32) + d["kzg_in2"][1]


def p_kzg_proof_batch(r):
    d, k = r.d, r.k
    blobs, zs, want_p, want_y = _kzg_batch_io(d)
    proofs, ys, st = Out(48 * 3), Out(32 * 3), Out(3)
    r.call(k, "ckzg_hip_compute_kzg_proof_batch", proofs.buf, ys.buf, st.buf, blobs, zs, U64(3), k.sp, allow=(1,))
    r.eq("status", st, statuses(3, {1}))
    r.eq("proofs", proofs, want_p, skips(48, {1}))
    r.eq("ys", ys, want_y, skips(32, {1}))


def p_kzg_proof_batch_device(r):
    d, k = r.d, r.k
    blobs, zs, want_p, want_y = _kzg_batch_io(d)
    d_blobs, d_zs, d_p, d_y, d_st = r.dev(blobs), r.dev(zs), r.dev_out(48 * 3), r.dev_out(32 * 3), r.dev_out(3)
    try:
        r.call(k, "ckzg_hip_compute_kzg_proof_batch_device", d_p, d_y, d_st, d_blobs, d_zs, U64(3), k.sp)
        r.eq("status", r.back("status", d_st, 3), statuses(3, {1}))
        r.eq("proofs", r.back("proofs", d_p, 48 * 3), want_p, skips(48, {1}))
        r.eq("ys", r.back("ys", d_y, 32 * 3), want_y, skips(32, {1}))
    finally:
        r.free(d_blobs, d_zs, d_p, d_y, d_st)


def p_blob_proof(r):
    d, k = r.d, r.k
    out = Out(48)
    r.call(k, "compute_blob_kzg_proof", out.buf, d["blobs"][0], d["cm"][0], k.sp)
    r.eq("compute_blob_kzg_proof", out, d["bproof"][0])
    proofs, st = Out(48 * 3), Out(3)
    r.call(k, "ckzg_hip_compute_blob_kzg_proof_batch", proofs.buf, st.buf, d["blobs"][0] + d["bad"] + d["blobs"][2],
           d["cm"][0] + d["cm"][1] + d["cm"][2], U64(3), k.sp, allow=(1,))
    r.eq("batch: status", st, statuses(3, {1}))
    r.eq("batch: proofs", proofs, d["bproof"][0] + bytes(48) + d["bproof"][2], skips(48, {1}))


def p_domain_proofs(r):
    d, k = r.d, r.k
    want = d["coset"][0][:4096 * 48]
    proofs, st = Out(4096 * 48), Out(1)
    r.call(k, "ckzg_hip_compute_domain_kzg_proofs_batch", proofs.buf, st.buf, d["blobs"][0], U64(1), k.sp)
    r.eq("status", st, b"\0")
    r.eq("proofs", proofs, want)
    d_blobs, d_p, d_st = r.dev(d["bad"] + d["blobs"][0]), r.dev_out(2 * 4096 * 48), r.dev_out(2)
    try:
        r.call(k, "ckzg_hip_compute_domain_kzg_proofs_batch_device", d_p, d_st, d_blobs, U64(2), k.sp)
        r.eq("device form: status", r.back("status", d_st, 2), b"\1\0")
        r.eq("device form: proofs", r.back("proofs", d_p, 2 * 4096 * 48)[4096 * 48:], want)
    finally:
        r.free(d_blobs, d_p, d_st)


def _coset_proofs_probe(e):
    def probe(r):
        d, k = r.d, r.k
        per, per_ev = (8192 >> e) * 48, 8192 * 32
        proofs, evals, st = Out(2 * per), Out(2 * per_ev), Out(2)
        r.call(k, "ckzg_hip_compute_coset_kzg_proofs_batch", proofs.buf, evals.buf, st.buf, d["bad"] + d["blobs"][0], U64(2),
               U32(e), k.sp, allow=(1,))
        r.eq("status", st, b"\1\0")
        r.eq("proofs", proofs, bytes(per) + d["coset"][e], [(0, per)])
        r.eq("evaluations", evals, bytes(per_ev) + d["evals0"], [(0, per_ev)])
        if e == 3:
            d_blobs, d_p, d_ev, d_st = r.dev(d["bad"] + d["blobs"][0]), r.dev_out(2 * per), r.dev_out(2 * per_ev), r.dev_out(2)
            try:
                r.call(k, "ckzg_hip_compute_coset_kzg_proofs_batch_device", d_p, d_ev, d_st, d_blobs, U64(2), U32(e), k.sp)
                r.eq("device form: status", r.back("status", d_st, 2), b"\1\0")
                r.eq("device form: proofs", r.back("proofs", d_p, 2 * per)[per:], d["coset"][e])
                r.eq("device form: evaluations", r.back("evaluations", d_ev, 2 * per_ev)[per_ev:], d["evals0"])
            finally:
                r.free(d_blobs, d_p, d_ev, d_st)
    return probe


# ---------------------------------------------------------------------------------------------------------------------
# cells, recover
# ---------------------------------------------------------------------------------------------------------------------

CELLS, CPROOFS = 128 * 2048, 128 * 48


def _cells_one(r, k, label):
    d = r.d
    cells, proofs = Out(CELLS), Out(CPROOFS)
    r.call(k, "compute_cells_and_kzg_proofs", cells.buf, proofs.buf, d["blobs"][0], k.sp)
    r.eq(label + ": cells", cells, d["cells"][0])
    r.eq(label + ": proofs", proofs, d["cproofs"][0])


def _cells_batch(r, k, label):
    d = r.d
    cells, proofs, st = Out(3 * CELLS), Out(3 * CPROOFS), Out(3)
    r.call(k, "ckzg_hip_compute_cells_and_kzg_proofs_batch", cells.buf, proofs.buf, st.buf,
           d["blobs"][0] + d["bad"] + d["blobs"][1], U64(3), k.sp, allow=(1,))
    r.eq(label + ": status", st, statuses(3, {1}))
    r.eq(label + ": cells", cells, d["cells"][0] + bytes(CELLS) + d["cells"][1], skips(CELLS, {1}))
    r.eq(label + ": proofs", proofs, d["cproofs"][0] + bytes(CPROOFS) + d["cproofs"][1], skips(CPROOFS, {1}))


def p_cells_direct(r):
    _cells_one(r, r.k, "direct path")


def p_cells_fk20(r):
    _cells_one(r, r.k2, "FK20 path (direct_max = 0)")


def p_cells_batch(r):
    _cells_batch(r, r.k, "3 blobs = direct_max + 2")          # (small tables: direct_max is 1)
    _cells_batch(r, r.k2, "3 blobs, direct_max = 0")


def p_cells_device(r):
    d, k = r.d, r.k
    d_blobs = r.dev(d["blobs"][0] + d["bad"] + d["blobs"][1])
    d_c, d_p, d_st = r.dev_out(3 * CELLS), r.dev_out(3 * CPROOFS), r.dev_out(3)
    try:
        r.call(k, "ckzg_hip_compute_cells_and_kzg_proofs_batch_device", d_c, d_p, d_st, d_blobs, U64(3), k.sp)
        r.eq("status", r.back("status", d_st, 3), statuses(3, {1}))
        r.eq("cells", r.back("cells", d_c, 3 * CELLS), d["cells"][0] + bytes(CELLS) + d["cells"][1], skips(CELLS, {1}))
        r.eq("proofs", r.back("proofs", d_p, 3 * CPROOFS), d["cproofs"][0] + bytes(CPROOFS) + d["cproofs"][1], skips(CPROOFS, {1}))
    finally:
        r.free(d_blobs, d_c, d_p, d_st)


def _held(cells, idx):
    return b"".join(cells[2048 * i:2048 * i + 2048] for i in idx)


HALF = list(range(0, 128, 2))
HUNDRED = [i for i in range(128) if i % 9 != 4][:100]


def p_recover_one(r):
    d, k = r.d, r.k
    for b, idx in ((0, HALF), (1, HUNDRED)):
        cells, proofs = Out(CELLS), Out(CPROOFS)
        r.call(k, "recover_cells_and_kzg_proofs", cells.buf, proofs.buf, (U64 * len(idx))(*idx), _held(d["cells"][b], idx),
               U64(len(idx)), k.sp)
        r.eq("from %d cells: cells" % len(idx), cells, d["cells"][b])
        r.eq("from %d cells: proofs" % len(idx), proofs, d["cproofs"][b])


def p_recover_batch(r):
    d, k = r.d, r.k
    rows = [_held(d["cells"][0], HALF), _held(d["cells"][1], HALF), _held(d["cells"][1], HALF)]
    rows[1] = rows[1][:2048 * 9 + 32 * 5] + R.to_bytes(32, "big") + rows[1][2048 * 9 + 32 * 6:]   # one value not canonical
    cells, proofs, st = Out(3 * CELLS), Out(3 * CPROOFS), Out(3)
    r.call(k, "ckzg_hip_recover_cells_and_kzg_proofs_batch", cells.buf, proofs.buf, st.buf, (U64 * 64)(*HALF), b"".join(rows),
           U64(64), U64(3), k.sp, allow=(1,))
    r.eq("status", st, statuses(3, {1}))
    r.eq("cells", cells, d["cells"][0] + bytes(CELLS) + d["cells"][1], skips(CELLS, {1}))
    r.eq("proofs", proofs, d["cproofs"][0] + bytes(CPROOFS) + d["cproofs"][1], skips(CPROOFS, {1}))


def p_recover_rows(r):
    """two rows that hold different cells, a row of 63 cells between them: its output rows are not written"""
    d, k = r.d, r.k
    short = HALF[:63]
    idx = HALF + short + HUNDRED
    held = _held(d["cells"][0], HALF) + _held(d["cells"][0], short) + _held(d["cells"][1], HUNDRED)
    start = [0, 64, 127, 227]
    cells, proofs, st = Out(3 * CELLS), Out(3 * CPROOFS), Out(3)
    r.call(k, "ckzg_hip_recover_cells_and_kzg_proofs_rows", cells.buf, proofs.buf, st.buf, (U64 * len(idx))(*idx), held,
           (U64 * 4)(*start), U64(3), k.sp, allow=(1,))
    r.eq("status", st, statuses(3, {1}))
    r.eq("cells", cells, d["cells"][0] + bytes([A5]) * CELLS + d["cells"][1])
    r.eq("proofs", proofs, d["cproofs"][0] + bytes([A5]) * CPROOFS + d["cproofs"][1])


def _recover_cosets_probe(e):
    def probe(r):
        d, k = r.d, r.k
        m, w = 8192 >> e, 32 << e
        sets = [list(range(0, m, 2)), [m], [c for c in range(m) if c % 5 != 1 or c >= m // 2]]   # the middle one: index out of range
        blobs = [0, 0, 1]
        idx, held, start = [], [], [0]
        for b, s in zip(blobs, sets):
            idx += s
            held.append(b"".join(d["cells"][b][w * c:w * c + w] for c in s if c < m) + (bytes(w) if s == [m] else b""))
            start.append(len(idx))
        evals, proofs, st = Out(3 * 8192 * 32), Out(3 * m * 48), Out(3)
        r.call(k, "ckzg_hip_recover_cosets_and_kzg_proofs_rows", evals.buf, proofs.buf, st.buf, (U64 * len(idx))(*idx),
               b"".join(held), (U64 * 4)(*start), U64(3), U32(e), k.sp, allow=(1,))
        r.eq("status", st, statuses(3, {1}))
        r.eq("evaluations", evals, d["cells"][0] + bytes([A5]) * (8192 * 32) + d["cells"][1])
        r.eq("proofs", proofs, d["coset"][e][0] + bytes([A5]) * (m * 48) + d["coset"][e][1])
    return probe


# ---------------------------------------------------------------------------------------------------------------------
# verify
# ---------------------------------------------------------------------------------------------------------------------

def p_verify_point(r):
    d, k = r.d, r.k
    for cm, z, y, p, want, st in d["items"]:
        ok = Out(1)
        r.call(k, "verify_kzg_proof", ok.buf, cm, z, y, p, k.sp, allow=(st,))
        if st == 0:
            r.eq("verify_kzg_proof, expected %s" % want, ok, bytes([want]))
        else:
            r.true("verify_kzg_proof of an invalid item says true", ok.raw != b"\1")


def _point_batch(r, name, with_stats):
    d, k = r.d, r.k
    it = d["items"]
    n = len(it)
    ok, st, stats = Out(n), Out(n), Out(24)
    args = [ok.buf, st.buf] + ([stats.buf] if with_stats else []) + [b"".join(t[i] for t in it) for i in range(4)] + [U64(n), k.sp]
    r.call(k, name, *args, allow=(1,))
    r.eq(name + ": status", st, bytes(t[5] for t in it))
    r.eq(name + ": verdicts", ok, bytes(int(t[4]) for t in it))
    r.true(name + ": bytes behind stats were written", stats.guard_ok())


def p_verify_point_batch(r):
    _point_batch(r, "ckzg_hip_verify_kzg_proof_batch", False)


def p_verify_point_locate(r):
    _point_batch(r, "ckzg_hip_verify_kzg_proof_batch_locate", True)


def p_verify_blob(r):
    d, k = r.d, r.k
    for b, pr, want in ((0, 0, True), (1, 0, False), (1, 1, True)):
        ok = Out(1)
        r.call(k, "verify_blob_kzg_proof", ok.buf, d["blobs"][b], d["cm"][b], d["bproof"][pr], k.sp)
        r.eq("verify_blob_kzg_proof, expected %s" % want, ok, bytes([want]))
    ch = k.compute_challenge(d["blobs"][0], d["cm"][0])
    r.eq("compute_challenge", ch, d["challenge"])


def _blob_batch_inputs(d, n, variant):
    """n blobs, all true; `spoilt`: blob 1 with blob 0's proof; `invalid`: blob 1 with a non-canonical element"""
    pick = [i % 3 for i in range(n)]
    blobs = [d["blobs"][p] for p in pick]
    proofs = [d["bproof"][p] for p in pick]
    if variant == "spoilt":
        proofs[1] = d["bproof"][0]
    if variant == "invalid":
        blobs[1] = d["bad"]
    return b"".join(blobs), b"".join(d["cm"][p] for p in pick), b"".join(proofs)


VARIANTS = (("true", 0, 1), ("spoilt", 0, 0), ("invalid", 1, None), ("true", 0, 1))   # (inputs, return value, verdict)


def _blob_batch(r, label, n, options=()):
    d, k = r.d, r.k
    for key, v in options:
        r.opt(key, v)
    try:
        for variant, ret, want in VARIANTS:
            blobs, cms, proofs = _blob_batch_inputs(d, n, variant)
            ok = Out(1)
            r.call(k, "verify_blob_kzg_proof_batch", ok.buf, blobs, cms, proofs, U64(n), k.sp, allow=(ret,))
            if want is None:
                r.true("%s, %s: an invalid batch says true" % (label, variant), ok.raw != b"\1" and ok.guard_ok())
            else:
                r.eq("%s, %s" % (label, variant), ok, bytes([want]))
    finally:
        for key, v in options:
            r.opt(key, DEFAULTS[key])


def p_verify_blob_batch3(r):
    _blob_batch(r, "3 blobs (host path)", 3)


def p_verify_blob_batch5(r):
    _blob_batch(r, "5 blobs", 5)


def p_verify_blob_batch_gpu_sha(r):
    _blob_batch(r, "5 blobs, gpu_sha_min = 1", 5, (("gpu_sha_min", 1),))


def p_verify_blob_batch_piped(r):
    _blob_batch(r, "4 blobs, verify_pipe_min = 2", 4, (("verify_pipe_min", 2),))


def p_verify_blob_batch_table(r):
    _blob_batch(r, "8 blobs (call-time table)", 8)
    _blob_batch(r, "8 blobs, verify_call_table = 0", 8, (("verify_call_table", 0),))


def p_verify_blob_device(r):
    d, k = r.d, r.k
    for variant, ret, want in VARIANTS:
        blobs, cms, proofs = _blob_batch_inputs(d, 5, variant)
        ptrs = [r.dev(blobs), r.dev(cms), r.dev(proofs)]
        try:
            ok = Out(1)
            r.call(k, "ckzg_hip_verify_blob_kzg_proof_batch_device", ok.buf, ptrs[0], ptrs[1], ptrs[2], U64(5), k.sp, allow=(ret,))
            if want is None:
                r.true("device form, %s: an invalid batch says true" % variant, ok.raw != b"\1" and ok.guard_ok())
            else:
                r.eq("device form, %s" % variant, ok, bytes([want]))
        finally:
            r.free(*ptrs)


def p_verify_blob_locate(r):
    d, k = r.d, r.k
    blobs, cms, proofs = _blob_batch_inputs(d, 5, "spoilt")
    ok, st, stats = Out(5), Out(5), Out(24)
    r.call(k, "ckzg_hip_verify_blob_kzg_proof_batch_locate", ok.buf, st.buf, stats.buf, blobs, cms, proofs, U64(5), k.sp)
    r.eq("status", st, bytes(5))
    r.eq("verdicts", ok, b"\1\0\1\1\1")
    r.true("bytes behind stats were written", stats.guard_ok())
    r.opt("locate_max_checks", 0)    # the hand-over to the per-lane check as soon as the root check fails
    try:
        ok, st = Out(5), Out(5)
        r.call(k, "ckzg_hip_verify_blob_kzg_proof_batch_locate", ok.buf, st.buf, None, blobs, cms, proofs, U64(5), k.sp)
        r.eq("locate_max_checks = 0: status", st, bytes(5))
        r.eq("locate_max_checks = 0: verdicts", ok, b"\1\0\1\1\1")
    finally:
        r.opt("locate_max_checks", DEFAULTS["locate_max_checks"])


# ---------------------------------------------------------------------------------------------------------------------
# cell verify
# ---------------------------------------------------------------------------------------------------------------------

def _flat(items):
    cms, idx, vals, proofs = zip(*items)
    return b"".join(cms), (U64 * len(idx))(*idx), b"".join(vals), b"".join(proofs)


def _bump_cell(item, element=9):
    cm, i, cell, pr = item
    return (cm, i, cell[:32 * element] + K.bump(cell[32 * element:32 * element + 32]) + cell[32 * element + 32:], pr)


def _cell_variants(items, at=1):
    """(label, items, return value, verdict): true, one bumped value, one index out of range, true again"""
    spoilt, invalid = list(items), list(items)
    spoilt[at] = _bump_cell(items[at])
    invalid[at] = (items[at][0], 128, items[at][2], items[at][3])
    return (("true", items, 0, 1), ("one bumped value", spoilt, 0, 0), ("index 128", invalid, 1, None), ("true again", items, 0, 1))


def _cell_batch(r, label, items, at=1):
    k = r.k
    for variant, its, ret, want in _cell_variants(items, at):
        ok = Out(1)
        cms, idx, cells, proofs = _flat(its)
        r.call(k, "verify_cell_kzg_proof_batch", ok.buf, cms, idx, cells, proofs, U64(len(its)), k.sp, allow=(ret,))
        if want is None:
            r.true("%s, %s: an invalid batch says true" % (label, variant), ok.raw != b"\1" and ok.guard_ok())
        else:
            r.eq("%s, %s" % (label, variant), ok, bytes([want]))


def p_cell_batch3(r):
    _cell_batch(r, "3 cells", r.d["cells3"])
    cms, ci, idx, cells, proofs = r.d["challenge_in"]
    r.eq("compute_verify_cell_kzg_proof_batch_challenge", r.k.compute_verify_cell_kzg_proof_batch_challenge(cms, ci, idx, cells, proofs),
         r.d["challenge"])


def p_cell_batch128(r):
    _cell_batch(r, "128 cells (call-time table), one of them twice", r.d["cells128"], at=70)


def p_cell_locate(r):
    d, k = r.d, r.k
    items = list(d["locate"])
    items[1] = _bump_cell(items[1])
    cm, i, cell, pr = items[2]
    items[2] = (cm, i, cell[:32 * 63] + R.to_bytes(32, "big"), pr)     # the last value not canonical
    n = len(items)
    ok, st, stats = Out(n), Out(n), Out(24)
    cms, idx, cells, proofs = _flat(items)
    r.call(k, "ckzg_hip_verify_cell_kzg_proof_batch_locate", ok.buf, st.buf, stats.buf, cms, idx, cells, proofs, U64(n), k.sp, allow=(1,))
    r.eq("status", st, b"\0\0\1\0\0")
    r.eq("verdicts", ok, b"\1\0\0\1\1")
    r.true("bytes behind stats were written", stats.guard_ok())


def _coset_verify_probe(e):
    def probe(r):
        d, k = r.d, r.k
        items = d["coset"][e]
        spoilt, invalid = list(items), list(items)
        spoilt[1] = _spoil_value(items[1])
        invalid[1] = _bad_value(items[1])
        for variant, its, ret, want in (("true", items, 0, 1), ("one bumped value", spoilt, 0, 0), ("a value not canonical", invalid, 1, None),
                                        ("true again", items, 0, 1)):
            ok = Out(1)
            cms, idx, vals, proofs = _flat(its)
            r.call(k, "ckzg_hip_verify_coset_kzg_proof_batch", ok.buf, cms, idx, vals, proofs, U64(len(its)), U32(e), k.sp, allow=(ret,))
            if want is None:
                r.true("%s: an invalid batch says true" % variant, ok.raw != b"\1" and ok.guard_ok())
            else:
                r.eq(variant, ok, bytes([want]))
        mixed = [items[0], spoilt[1], _bad_value(items[2]), items[3]]
        ok, st, stats = Out(4), Out(4), Out(24)
        cms, idx, vals, proofs = _flat(mixed)
        r.call(k, "ckzg_hip_verify_coset_kzg_proof_batch_locate", ok.buf, st.buf, stats.buf, cms, idx, vals, proofs, U64(4), U32(e),
               k.sp, allow=(1,))
        r.eq("locate: status", st, b"\0\0\1\0")
        r.eq("locate: verdicts", ok, b"\1\0\0\1")
        r.true("locate: bytes behind stats were written", stats.guard_ok())
    return probe


# ---------------------------------------------------------------------------------------------------------------------
# groups: true, false, invalid, true; the commitment of blob 0 is in every group
# ---------------------------------------------------------------------------------------------------------------------

WANT_OK, WANT_ST = b"\1\0\0\1", b"\0\0\1\0"


def _groups_call(r, name, flat_args, start, extra=()):
    k = r.k
    ok, st = Out(4), Out(4)
    r.call(k, name, ok.buf, st.buf, *flat_args, (U64 * 5)(*start), U64(4), *extra, k.sp, allow=(1,))
    r.eq("status", st, WANT_ST)
    r.eq("verdicts", ok, WANT_OK)


def _item_groups(items, spoil, invalid):
    a, b, c, e = items[:4]
    groups = [[a, b, c], [a, spoil(b)], [c, invalid(b), a], [e, a]]
    flat = [t for g in groups for t in g]
    start = [0]
    for g in groups:
        start.append(start[-1] + len(g))
    return flat, start


def p_cell_groups(r):
    flat, start = _item_groups(r.d["cell_items"], _bump_cell, lambda t: (t[0], 128, t[2], t[3]))
    _groups_call(r, "ckzg_hip_verify_cell_kzg_proof_batch_groups", _flat(flat), start)


def _coset_groups_probe(e):
    def probe(r):
        flat, start = _item_groups(r.d["coset"][e], _spoil_value, _bad_value)
        _groups_call(r, "ckzg_hip_verify_coset_kzg_proof_batch_groups", _flat(flat), start, (U32(e),))
    return probe


def p_blob_groups(r):
    d = r.d
    B, cm, pr = d["blobs"], d["cm"], d["bproof"]
    blobs = [B[0], B[1], B[0], B[2], d["bad"], B[0], B[2], B[0]]
    cms = [cm[0], cm[1], cm[0], cm[2], cm[1], cm[0], cm[2], cm[0]]
    proofs = [pr[0], pr[1], pr[0], pr[1], pr[1], pr[0], pr[2], pr[0]]      # (group 1: blob 2 with blob 1's proof)
    _groups_call(r, "ckzg_hip_verify_blob_kzg_proof_batch_groups", (b"".join(blobs), b"".join(cms), b"".join(proofs)), [0, 2, 4, 6, 8])


def p_blob_cell_groups(r):
    d = r.d
    B, cm, cp = d["blobs"], d["cm"], d["cproofs"]
    swapped = list(cp[1])
    swapped[17], swapped[18] = swapped[18], swapped[17]
    blobs = [B[0], B[0], B[1], d["bad"], B[1], B[0]]
    cms = [cm[0], cm[0], cm[1], cm[1], cm[1], cm[0]]
    proofs = cp[0] + cp[0] + swapped + cp[1] + cp[1] + cp[0]
    _groups_call(r, "ckzg_hip_verify_blob_cell_kzg_proof_batch_groups", (b"".join(blobs), b"".join(cms), b"".join(proofs)), [0, 1, 3, 4, 6])


# ---------------------------------------------------------------------------------------------------------------------
# G1 utilities: g1_t (Jacobian) outputs are compared as points, by the oracle
# ---------------------------------------------------------------------------------------------------------------------

_ORACLE = []


def _points_eq(r, label, out, want):
    if not _ORACLE:
        _ORACLE.append(K.OracleG1())
    g1 = _ORACLE[0]
    r.true("%s: bytes behind the output were written" % label, out.guard_ok())
    raw = out.raw
    for i, w in enumerate(want):
        if not g1.eq(raw[144 * i:144 * i + 144], w):
            r.fails.append("%s: point %d of %d differs" % (label, i, len(want)))
            return


def _g1_fft_probe(n):
    def probe(r):
        d, k = r.d["fft"][n], r.k
        for inverse in (0, 1):
            out = Out(144 * n)
            r.call(k, "ckzg_hip_g1_fft", out.buf, b"".join(d["in"]), U64(n), U64(1), INT(inverse), k.sp)
            _points_eq(r, "n = %d, inverse = %d" % (n, inverse), out, d[inverse])
    return probe


def _g1_prefix_probe(n):
    def probe(r):
        d, k = r.d["prefix"][n], r.k
        out = Out(144 * n)
        r.call(k, "ckzg_hip_g1_prefix_sums", out.buf, b"".join(d["in"]), U64(n), k.sp)
        _points_eq(r, "%d points" % n, out, d["out"])
    return probe


def p_g1_lincomb(r):
    d, k = r.d["lincomb"], r.k
    for algo in (0, 1, 2):
        out = Out(144)
        r.call(k, "ckzg_hip_g1_lincomb", out.buf, b"".join(d["in"]), b"".join(d["coeffs"]), U64(len(d["in"])), INT(algo), k.sp)
        _points_eq(r, "algo %d" % algo, out, [d["out"]])


# ---------------------------------------------------------------------------------------------------------------------
# the table: family -> (probe, the exported symbols it calls, function)
# ---------------------------------------------------------------------------------------------------------------------

PROBES = {
    "commit": [
        ("one_blob", ("blob_to_kzg_commitment",), p_commit_one),
        ("batch_5", ("ckzg_hip_blob_to_kzg_commitment_batch",), p_commit_batch5),
        ("batch_65", ("ckzg_hip_blob_to_kzg_commitment_batch",), p_commit_batch65),
        ("batch_133_deferred", ("ckzg_hip_blob_to_kzg_commitment_batch",), p_commit_batch133),
        ("batch_device_5", ("ckzg_hip_blob_to_kzg_commitment_batch_device",), p_commit_device),
        ("four_threads", ("blob_to_kzg_commitment",), p_commit_threads),
    ],
    "proofs": [
        ("kzg_proof", ("compute_kzg_proof",), p_kzg_proof),
        ("kzg_proof_batch_3", ("ckzg_hip_compute_kzg_proof_batch",), p_kzg_proof_batch),
        ("kzg_proof_batch_device_3", ("ckzg_hip_compute_kzg_proof_batch_device",), p_kzg_proof_batch_device),
        ("blob_proof", ("compute_blob_kzg_proof", "ckzg_hip_compute_blob_kzg_proof_batch"), p_blob_proof),
        ("domain_proofs", ("ckzg_hip_compute_domain_kzg_proofs_batch", "ckzg_hip_compute_domain_kzg_proofs_batch_device"), p_domain_proofs),
        ("coset_proofs_e0", ("ckzg_hip_compute_coset_kzg_proofs_batch",), _coset_proofs_probe(0)),
        ("coset_proofs_e3", ("ckzg_hip_compute_coset_kzg_proofs_batch", "ckzg_hip_compute_coset_kzg_proofs_batch_device"), _coset_proofs_probe(3)),
        ("coset_proofs_e6", ("ckzg_hip_compute_coset_kzg_proofs_batch",), _coset_proofs_probe(6)),
    ],
    "cells": [
        ("one_direct", ("compute_cells_and_kzg_proofs",), p_cells_direct),
        ("one_fk20", ("compute_cells_and_kzg_proofs",), p_cells_fk20),
        ("batch_3", ("ckzg_hip_compute_cells_and_kzg_proofs_batch",), p_cells_batch),
        ("batch_device_3", ("ckzg_hip_compute_cells_and_kzg_proofs_batch_device",), p_cells_device),
    ],
    "recover": [
        ("one_64_and_100", ("recover_cells_and_kzg_proofs",), p_recover_one),
        ("batch_3", ("ckzg_hip_recover_cells_and_kzg_proofs_batch",), p_recover_batch),
        ("rows", ("ckzg_hip_recover_cells_and_kzg_proofs_rows",), p_recover_rows),
        ("cosets_rows_e0", ("ckzg_hip_recover_cosets_and_kzg_proofs_rows",), _recover_cosets_probe(0)),
        ("cosets_rows_e3", ("ckzg_hip_recover_cosets_and_kzg_proofs_rows",), _recover_cosets_probe(3)),
        ("cosets_rows_e6", ("ckzg_hip_recover_cosets_and_kzg_proofs_rows",), _recover_cosets_probe(6)),
    ],
    "verify": [
        ("point", ("verify_kzg_proof",), p_verify_point),
        ("point_batch_5", ("ckzg_hip_verify_kzg_proof_batch",), p_verify_point_batch),
        ("point_locate_5", ("ckzg_hip_verify_kzg_proof_batch_locate",), p_verify_point_locate),
        ("blob", ("verify_blob_kzg_proof", "compute_challenge"), p_verify_blob),
        ("blob_batch_3", ("verify_blob_kzg_proof_batch",), p_verify_blob_batch3),
        ("blob_batch_5", ("verify_blob_kzg_proof_batch",), p_verify_blob_batch5),
        ("blob_batch_5_gpu_sha", ("verify_blob_kzg_proof_batch",), p_verify_blob_batch_gpu_sha),
        ("blob_batch_4_piped", ("verify_blob_kzg_proof_batch",), p_verify_blob_batch_piped),
        ("blob_batch_8_table", ("verify_blob_kzg_proof_batch",), p_verify_blob_batch_table),
        ("blob_batch_device_5", ("ckzg_hip_verify_blob_kzg_proof_batch_device",), p_verify_blob_device),
        ("blob_locate_5", ("ckzg_hip_verify_blob_kzg_proof_batch_locate",), p_verify_blob_locate),
    ],
    "cell_verify": [
        ("cells_3", ("verify_cell_kzg_proof_batch", "compute_verify_cell_kzg_proof_batch_challenge"), p_cell_batch3),
        ("cells_128_table", ("verify_cell_kzg_proof_batch",), p_cell_batch128),
        ("cell_locate_5", ("ckzg_hip_verify_cell_kzg_proof_batch_locate",), p_cell_locate),
        ("cosets_e0", ("ckzg_hip_verify_coset_kzg_proof_batch", "ckzg_hip_verify_coset_kzg_proof_batch_locate"), _coset_verify_probe(0)),
        ("cosets_e3", ("ckzg_hip_verify_coset_kzg_proof_batch", "ckzg_hip_verify_coset_kzg_proof_batch_locate"), _coset_verify_probe(3)),
        ("cosets_e6", ("ckzg_hip_verify_coset_kzg_proof_batch", "ckzg_hip_verify_coset_kzg_proof_batch_locate"), _coset_verify_probe(6)),
    ],
    "groups": [
        ("cell_groups", ("ckzg_hip_verify_cell_kzg_proof_batch_groups",), p_cell_groups),
        ("coset_groups_e0", ("ckzg_hip_verify_coset_kzg_proof_batch_groups",), _coset_groups_probe(0)),
        ("coset_groups_e3", ("ckzg_hip_verify_coset_kzg_proof_batch_groups",), _coset_groups_probe(3)),
        ("coset_groups_e6", ("ckzg_hip_verify_coset_kzg_proof_batch_groups",), _coset_groups_probe(6)),
        ("blob_groups", ("ckzg_hip_verify_blob_kzg_proof_batch_groups",), p_blob_groups),
        ("blob_cell_groups", ("ckzg_hip_verify_blob_cell_kzg_proof_batch_groups",), p_blob_cell_groups),
    ],
    "g1": [
        ("fft_2", ("ckzg_hip_g1_fft",), _g1_fft_probe(2)),
        ("fft_64", ("ckzg_hip_g1_fft",), _g1_fft_probe(64)),
        ("fft_256", ("ckzg_hip_g1_fft",), _g1_fft_probe(256)),
        ("prefix_sums_1", ("ckzg_hip_g1_prefix_sums",), _g1_prefix_probe(1)),
        ("prefix_sums_300", ("ckzg_hip_g1_prefix_sums",), _g1_prefix_probe(300)),
        ("lincomb_130", ("ckzg_hip_g1_lincomb",), p_g1_lincomb),
    ],
}
EXPECTED = {"commit": expected_commit, "proofs": expected_proofs, "cells": expected_cells, "recover": expected_recover,
            "verify": expected_verify, "cell_verify": expected_cell_verify, "groups": expected_groups, "g1": expected_g1}
NEEDS_FK20_SETTINGS = ("cells",)


def probed_symbols():
    return {s for probes in PROBES.values() for _, symbols, _ in probes for s in symbols}


# ---------------------------------------------------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------------------------------------------------

def main(family, expected_path, report_path, fills=POISONS):
    from kzg_ctypes import HIP_SO, Kzg
    with open(expected_path, "rb") as f:
        data = pickle.load(f)[family]
    report = {"family": family, "runs": {}, "seconds": {}, "notes": {}, "stopped": None, "done": False}

    def save():
        tmp = report_path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(report, f)
        os.replace(tmp, report_path)

    save()
    rt = hip_runtime()
    lib = C.CDLL(HIP_SO)
    setopt = lib.ckzg_hip_set_option
    setopt.restype, setopt.argtypes = C.c_int, [C.c_char_p, C.c_int64]
    try:
        for poison in fills:
            key = "0x%02X" % poison
            run = Run(rt, data)
            report["runs"][key] = {}
            where = "load"
            t0 = time.time()
            try:
                # settings of this run's own, loaded with the fill byte already set: the first probe is a first call
                if setopt(b"poison_temporaries", poison) != 0:
                    run.stop("option poison_temporaries = %d refused" % poison)
                run.k = Kzg(HIP_SO, "", precompute=0, options=SMALL_TABLES)
                if family in NEEDS_FK20_SETTINGS:
                    run.k2 = Kzg(HIP_SO, "", precompute=0, options=dict(SMALL_TABLES, direct_max=0))
                    setopt(b"direct_max", -1)
                for name, _, fn in PROBES[family]:
                    where = name
                    sys.stderr.write("[poison] %s %s %s\n" % (family, key, name))
                    sys.stderr.flush()
                    run.fails = []
                    fn(run)
                    e = rt.hipDeviceSynchronize()
                    if e != 0:
                        run.stop("HIP error %d after the probe" % e)
                    report["runs"][key][name] = run.fails
                    if run.notes:
                        report["notes"][key] = run.notes
                    save()
            except Exception as e:   # Stop, a KzgError of the binding, anything: nothing further on the GPU
                report["stopped"] = {"poison": key, "probe": where, "why": "%s: %s" % (type(e).__name__, e)}
                save()
                return 1
            finally:
                report["seconds"][key] = round(time.time() - t0, 3)
            for k in (run.k, run.k2):
                if k is not None:
                    k.close()
        report["done"] = True
        save()
        return 0
    finally:
        if report["stopped"] is None:   # (after a stop the child makes no further call into the library: it ends)
            for k, v in DEFAULTS.items():
                setopt(k.encode(), v)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3],
                  tuple(int(v) for v in sys.argv[4].split(",")) if len(sys.argv) > 4 else POISONS))
