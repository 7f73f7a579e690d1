"""Runs under LD_PRELOAD=failalloc.so (tests/test_gpu_point_proofs_alloc.py starts it): every device / page-locked
allocation, then every stream and event creation, of ckzg_hip_verify_kzg_proof_batch is made to fail in turn, once
and (for allocations) from then on.  What must hold each time: the call returns C_KZG_MALLOC (allocations) or
C_KZG_ERROR / C_KZG_MALLOC (streams, events) -- or its normal result, where nothing it needed failed --, never a crash;
no device memory is kept; the same call right after on the same settings gives the right verdicts.  The batch spans
two chunks of the call (more items than one chunk holds) and includes an invalid item.  Prints one JSON line."""
import ctypes as C
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from kzg_ctypes import Kzg, HIP_SO  # noqa: E402

LIB = os.environ.get("CKZG_HIP_SO") or HIP_SO
fa = C.CDLL(os.environ["FAILALLOC_SO"])
fa.failalloc_arm.argtypes = [C.c_long, C.c_int]
fa.failalloc_class.argtypes = [C.c_int]
fa.failalloc_fired.restype = C.c_long
fa.failalloc_seen.restype = C.c_long
fa.failalloc_free_bytes.restype = C.c_longlong
C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC = 1, 2, 3
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
CHUNK = 65536   # ckzg_api2.hip: verify_point_proofs_on


def fr(v):
    return (v % R).to_bytes(32, "big")


def load():
    return Kzg(LIB, "", precompute=0)


k0 = load()
rnd = random.Random(5)
tuples = []
for i in range(4):
    blob = b"".join(fr(rnd.randrange(R)) for _ in range(4096))
    c = k0.blob_to_kzg_commitment(blob)
    z = fr(rnd.randrange(R))
    p, y = k0.compute_kzg_proof(blob, z)
    tuples.append((c, z, y, p))
k0.close()
N = CHUNK + 70
items = []
for i in range(N):
    c, z, y, p = tuples[i % 4]
    if i % 3 == 1:
        y = fr(int.from_bytes(y, "big") + 1)   # a wrong evaluation: verdict false
    items.append((c, z, y, p))
items[CHUNK + 5] = (items[CHUNK + 5][0], R.to_bytes(32, "big"), items[CHUNK + 5][2], items[CHUNK + 5][3])  # z >= r
ARGS = [b"".join(t[j] for t in items) for j in range(4)]


def call(k):
    ok = (C.c_bool * N)()
    st = (C.c_uint8 * N)()
    ret = k.lib.ckzg_hip_verify_kzg_proof_batch(ok, st, ARGS[0], ARGS[1], ARGS[2], ARGS[3], C.c_uint64(N), k.sp)
    return ret, bytes(ok), bytes(st)


problems = []
LEAK = 4 << 20
report = {}


def walk(cls, allowed, stickies, key):
    fa.failalloc_class(cls)
    k = load()
    want = call(k)
    k.close()
    if want[0] != C_KZG_BADARGS or want[2].count(C_KZG_BADARGS) != 1:
        problems.append("%s: unarmed call gave %d with %d invalid items" % (key, want[0], want[2].count(C_KZG_BADARGS)))
    base = fa.failalloc_free_bytes()
    for sticky in stickies:
        fired_total, seen_unarmed = 0, None
        for nth in range(0, 64):
            sys.stderr.write("[failalloc] %s: failure %d, sticky=%d\n" % (key, nth, sticky))
            k = load()
            fa.failalloc_arm(nth, sticky)
            got = call(k)
            fired, seen = fa.failalloc_fired(), fa.failalloc_seen()
            fa.failalloc_disarm()
            what = "%s %d failed (sticky=%d)" % (key, nth, sticky)
            if not fired:
                seen_unarmed = seen
                if got != want:
                    problems.append("%s: unarmed result differs" % key)
                k.close()
                break
            fired_total += 1
            if got[0] not in allowed and got != want:
                problems.append("%s -> C_KZG_RET %d" % (what, got[0]))
            if got[0] == C_KZG_BADARGS and got != want:
                problems.append("%s -> a result, but a wrong one" % what)
            after = call(k)   # the same settings, the same call, right after the failure
            if after != want:
                problems.append("%s: call after -> C_KZG_RET %d%s" % (what, after[0], "" if after[0] != want[0] else ", wrong verdicts"))
            k.close()
            d = base - fa.failalloc_free_bytes()
            if d > LEAK:
                problems.append("%s: %d bytes of device memory not returned" % (what, d))
        report.setdefault(key, {})["sticky" if sticky else "single"] = {"seen": seen_unarmed, "failures_injected": fired_total}
    fa.failalloc_class(0)


walk(0, (C_KZG_MALLOC,), (0, 1), "allocations")
walk(1, (C_KZG_ERROR, C_KZG_MALLOC), (0,), "streams_events")
print(json.dumps({"report": report, "problems": problems}))
