"""Runs under LD_PRELOAD=failalloc.so (tests/test_point_openings_alloc.py starts it): every device / page-locked
allocation, then every stream and event creation, of ckzg_hip_compute_kzg_proof_batch and of its _device form is made to
fail in turn, once and (for allocations) from then on.  What must hold each time: the call returns C_KZG_MALLOC
(allocations) or C_KZG_ERROR / C_KZG_MALLOC (streams, events) -- or its normal result, where nothing it needed failed
--, never a crash; no device memory is kept; the same call right after on the same settings gives the right results.
The batch spans two chunks of the call, mixes domain-point and random z and holds one invalid item.  The device form's
own buffers are allocated before any failure is armed.  Prints one JSON line."""
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
rt = C.CDLL("/opt/rocm/lib/libamdhip64.so")
rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC = 1, 2, 3
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
CHUNK = 256   # ckzg_api2.hip: POINT_CHUNK
BLOB = 131072


def fr(v):
    return (v % R).to_bytes(32, "big")


def load():
    return Kzg(LIB, "", precompute=0)


rnd = random.Random(9)
base_blobs = [b"".join(fr(rnd.randrange(R)) for _ in range(4096)) for _ in range(3)]
w = pow(7, (R - 1) // 4096, R)
N = CHUNK + 6
zs = [fr(pow(w, rnd.randrange(4096), R)) if i % 2 else fr(rnd.randrange(R)) for i in range(N)]
zs[CHUNK + 2] = R.to_bytes(32, "big")   # z >= r: the invalid item
BLOBS = b"".join(base_blobs[i % 3] for i in range(N))
ZS = b"".join(zs)

dev = []
for size in (48 * N, 32 * N, N, BLOB * N, 32 * N):
    p = C.c_void_p()
    assert rt.hipMalloc(C.byref(p), size) == 0
    dev.append(p)
assert rt.hipMemcpy(dev[3], C.c_char_p(BLOBS), len(BLOBS), 1) == 0
assert rt.hipMemcpy(dev[4], C.c_char_p(ZS), len(ZS), 1) == 0


def call_host(k):
    proofs, ys, st = C.create_string_buffer(48 * N), C.create_string_buffer(32 * N), (C.c_uint8 * N)()
    ret = k.lib.ckzg_hip_compute_kzg_proof_batch(proofs, ys, st, BLOBS, ZS, C.c_uint64(N), k.sp)
    return ret, proofs.raw, ys.raw, bytes(st)


def call_device(k):
    for p, size in zip(dev[:3], (48 * N, 32 * N, N)):
        assert rt.hipMemset(p, 0, size) == 0
    ret = k.lib.ckzg_hip_compute_kzg_proof_batch_device(dev[0], dev[1], dev[2], dev[3], dev[4], C.c_uint64(N), k.sp)
    out = []
    for p, size in zip(dev[:3], (48 * N, 32 * N, N)):
        h = C.create_string_buffer(size)
        assert rt.hipMemcpy(h, p, size, 2) == 0
        out.append(h.raw)
    return (ret, *out)


def valid_part(res):
    """the return value, the statuses and the outputs of the valid items (an invalid item's outputs are unspecified)"""
    ret, proofs, ys, st = res
    keep = [i for i in range(N) if i != CHUNK + 2]
    return ret, st, [proofs[48 * i:48 * i + 48] for i in keep], [ys[32 * i:32 * i + 32] for i in keep]


# a load, both calls and a free before the walks: what the first free of the process keeps (the runtime's own) is then
# in the base figure of every walk
k0 = load()
call_host(k0)
call_device(k0)
k0.close()

problems = []
LEAK = 4 << 20
report = {}


def walk(cls, allowed, stickies, key, call, want_ret):
    fa.failalloc_class(cls)
    k = load()
    want = valid_part(call(k))
    k.close()
    if want[0] != want_ret or want[1].count(C_KZG_BADARGS) != 1:
        problems.append("%s: unarmed call gave %d with %d invalid items" % (key, want[0], want[1].count(C_KZG_BADARGS)))
    base = fa.failalloc_free_bytes()
    for sticky in stickies:
        fired_total, seen_unarmed = 0, None
        for nth in range(0, 64):
            sys.stderr.write("[failalloc] %s: failure %d, sticky=%d\n" % (key, nth, sticky))
            k = load()
            fa.failalloc_arm(nth, sticky)
            got = valid_part(call(k))
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
            if got[0] == want_ret and got != want:
                problems.append("%s -> a result, but a wrong one" % what)
            after = valid_part(call(k))   # the same settings, the same call, right after the failure
            if after != want:
                problems.append("%s: call after -> C_KZG_RET %d%s" % (what, after[0], "" if after[0] != want[0] else ", wrong results"))
            k.close()
            d = base - fa.failalloc_free_bytes()
            if d > LEAK:
                problems.append("%s: %d bytes of device memory not returned" % (what, d))
        report.setdefault(key, {})["sticky" if sticky else "single"] = {"seen": seen_unarmed, "failures_injected": fired_total}
    fa.failalloc_class(0)


for form, call, want_ret in (("host", call_host, C_KZG_BADARGS), ("device", call_device, 0)):
    walk(0, (C_KZG_MALLOC,), (0, 1), form + "_allocations", call, want_ret)
    walk(1, (C_KZG_ERROR, C_KZG_MALLOC), (0,), form + "_streams_events", call, want_ret)
print(json.dumps({"report": report, "problems": problems}))
