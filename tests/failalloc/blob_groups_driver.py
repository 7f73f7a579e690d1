"""Runs under LD_PRELOAD=failalloc.so (tests/test_gpu_blob_groups_alloc.py starts it): every device / page-locked
allocation, then every stream and event creation, of ckzg_hip_verify_blob_kzg_proof_batch_groups is made to fail in
turn, once and (for allocations) from then on.  What must hold each time: the call returns C_KZG_MALLOC (allocations)
or C_KZG_ERROR / C_KZG_MALLOC (streams, events) -- or its normal result, where nothing it needed failed --, never a
crash; no device memory is kept; the same call right after on the same settings gives the right verdicts.  The call
has a valid, a wrong, an invalid and an empty group among its twelve.  Prints one JSON line."""
import ctypes as C
import json
import random

from walk import C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC, R, fr, load, problems, report, walk

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


def want_ok(key, want):
    if want[0] != C_KZG_BADARGS or [bool(v) for v in want[1]] != EXPECT_OK or list(want[2]) != [int(g == 7) for g in range(G)]:
        return "%s: unarmed call gave %d, verdicts %s, status %s" % (key, want[0], list(want[1]), list(want[2]))
    return None


walk(0, (C_KZG_MALLOC,), (0, 1), "allocations", call, want_ok)
walk(1, (C_KZG_ERROR, C_KZG_MALLOC), (0,), "streams_events", call, want_ok)
print(json.dumps({"report": report, "problems": problems}))
