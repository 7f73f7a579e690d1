"""Runs under LD_PRELOAD=failalloc.so (tests/test_gpu_point_proofs_alloc.py starts it): every device / page-locked
allocation, then every stream and event creation, of ckzg_hip_verify_kzg_proof_batch is made to fail in turn, once
and (for allocations) from then on.  What must hold each time: the call returns C_KZG_MALLOC (allocations) or
C_KZG_ERROR / C_KZG_MALLOC (streams, events) -- or its normal result, where nothing it needed failed --, never a crash;
no device memory is kept; the same call right after on the same settings gives the right verdicts.  The batch spans
two chunks of the call (more items than one chunk holds) and includes an invalid item.  Prints one JSON line."""
import ctypes as C
import json
import random

from walk import C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC, R, fr, load, problems, report, walk

CHUNK = 65536   # ckzg_api2.hip: verify_point_proofs_on

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


def want_ok(key, want):
    if want[0] != C_KZG_BADARGS or want[2].count(C_KZG_BADARGS) != 1:
        return "%s: unarmed call gave %d with %d invalid items" % (key, want[0], want[2].count(C_KZG_BADARGS))
    return None


walk(0, (C_KZG_MALLOC,), (0, 1), "allocations", call, want_ok)
walk(1, (C_KZG_ERROR, C_KZG_MALLOC), (0,), "streams_events", call, want_ok)
print(json.dumps({"report": report, "problems": problems}))
