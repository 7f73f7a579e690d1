"""Runs under LD_PRELOAD=failalloc.so (tests/test_gpu_blob_groups_alloc.py starts it): every device / page-locked
allocation, then every stream and event creation, of ckzg_hip_verify_blob_kzg_proof_batch_groups is made to fail in
turn, once and (for allocations) from then on.  What must hold each time: the call returns C_KZG_MALLOC (allocations)
or C_KZG_ERROR / C_KZG_MALLOC (streams, events) -- or its normal result, where nothing it needed failed --, never a
crash; no device memory is kept; the same call right after on the same settings gives the right verdicts.  The call
has a valid, a wrong, an invalid and an empty group among its twelve.  Prints one JSON line."""
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


def fr(v):
    return (v % R).to_bytes(32, "big")


def load():
    return Kzg(LIB, "", precompute=0)


k0 = load()
rnd = random.Random(5)
rows = []
for i in range(2):
    blob = b"".join(fr(rnd.randrange(R)) for _ in range(4096))
    cm = k0.blob_to_kzg_commitment(blob)
    rows.append((blob, cm, k0.compute_blob_kzg_proof(blob, cm)))
k0.close()
G = 12
groups = []
for g in range(G):
    n = 0 if g == 4 else 3
    groups.append([[rows[(g + j) % 2][k] for j in range(n)] for k in range(3)])
groups[2][2][0], groups[2][2][1] = groups[2][2][1], groups[2][2][0]   # two proofs swapped: verdict false
groups[7][0][1] = groups[7][0][1][:32] + R.to_bytes(32, "big") + groups[7][0][1][64:]   # a field element >= r: invalid
EXPECT_OK = [g not in (2, 7) for g in range(G)]
START = [0]
for grp in groups:
    START.append(START[-1] + len(grp[0]))
FLAT = [[x for grp in groups for x in grp[k]] for k in range(3)]
ARGS = [b"".join(FLAT[0]), b"".join(FLAT[1]), b"".join(FLAT[2]), (C.c_uint64 * (G + 1))(*START)]


def call(k):
    ok = (C.c_bool * G)()
    st = (C.c_uint8 * G)()
    ret = k.lib.ckzg_hip_verify_blob_kzg_proof_batch_groups(ok, st, ARGS[0], ARGS[1], ARGS[2], ARGS[3], C.c_uint64(G), k.sp)
    return ret, bytes(ok), bytes(st)


problems = []
LEAK = 4 << 20
report = {}


def walk(cls, allowed, stickies, key):
    fa.failalloc_class(cls)
    k = load()
    want = call(k)
    k.close()
    if want[0] != C_KZG_BADARGS or [bool(v) for v in want[1]] != EXPECT_OK or list(want[2]) != [int(g == 7) for g in range(G)]:
        problems.append("%s: unarmed call gave %d, verdicts %s, status %s" % (key, want[0], list(want[1]), list(want[2])))
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
