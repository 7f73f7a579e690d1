"""Runs under LD_PRELOAD=failalloc.so (tests/test_gpu_locate_alloc.py starts it): every device / page-locked
allocation, then every stream and event creation, of ckzg_hip_verify_kzg_proof_batch_locate,
ckzg_hip_verify_blob_kzg_proof_batch_locate and ckzg_hip_g1_prefix_sums is made to fail in turn, once and (for
allocations) from then on.  What must hold each time: the call returns C_KZG_MALLOC (allocations) or C_KZG_ERROR /
C_KZG_MALLOC (streams, events) -- or its normal result, where nothing it needed failed --, never a crash; no device
memory is kept; the same call right after on the same settings gives the right result.  The verify batches hold a false
and an invalid item and run with locate_max_checks = 0, so that the hand-over to the per-lane check is part of the call.
Prints one JSON line."""
import ctypes as C
import hashlib
import json
import random

from walk import C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC, R, fr, load, problems, report, walk

k0 = load()
assert k0.lib.ckzg_hip_set_option(b"locate_max_checks", C.c_int64(0)) == 0
rnd = random.Random(5)
blobs = [b"".join(b"\x00" + hashlib.sha256(b"locwalk%d/%d" % (i, j)).digest()[:31] for j in range(4096)) for i in range(3)]
cms = [k0.blob_to_kzg_commitment(b) for b in blobs]
bproofs = [k0.compute_blob_kzg_proof(b, c) for b, c in zip(blobs, cms)]
tuples = []
for i in range(3):
    z = fr(rnd.randrange(R))
    p, y = k0.compute_kzg_proof(blobs[i], z)
    tuples.append((cms[i], z, y, p))
k0.close()

N = 70
items = [tuples[i % 3] for i in range(N)]
items[11] = (items[11][0], items[11][1], fr(int.from_bytes(items[11][2], "big") + 1), items[11][3])   # a wrong evaluation
items[65] = (items[65][0], R.to_bytes(32, "big"), items[65][2], items[65][3])                           # z >= r
ARGS = [b"".join(t[j] for t in items) for j in range(4)]
WANT_OK = bytes(0 if i in (11, 65) else 1 for i in range(N))


def call_points(k):
    ok, st, stats = (C.c_bool * N)(), (C.c_uint8 * N)(), (C.c_uint64 * 3)()
    ret = k.lib.ckzg_hip_verify_kzg_proof_batch_locate(ok, st, stats, ARGS[0], ARGS[1], ARGS[2], ARGS[3], C.c_uint64(N), k.sp)
    return ret, bytes(ok), bytes(st)


def want_points(key, want):
    if want[0] != C_KZG_BADARGS or want[1] != WANT_OK or want[2].count(C_KZG_BADARGS) != 1:
        return "%s: unarmed call gave %d, verdicts %r" % (key, want[0], want[1])
    return None


bad_blob = bytearray(blobs[2])
bad_blob[32 * 5:32 * 6] = R.to_bytes(32, "big")
BLOBS = blobs[0] + blobs[1] + bytes(bad_blob)
BC, BP = cms[0] + cms[1] + cms[2], bproofs[0] + bproofs[0] + bproofs[2]   # the second blob with the first one's proof


def call_blobs(k):
    ok, st, stats = (C.c_bool * 3)(), (C.c_uint8 * 3)(), (C.c_uint64 * 3)()
    ret = k.lib.ckzg_hip_verify_blob_kzg_proof_batch_locate(ok, st, stats, BLOBS, BC, BP, C.c_uint64(3), k.sp)
    return ret, bytes(ok), bytes(st)


def want_blobs(key, want):
    if want != (C_KZG_BADARGS, bytes([1, 0, 0]), bytes([0, 0, 1])):
        return "%s: unarmed call gave %r" % (key, want)
    return None


# 300 points: two tiles of the scan.  g1_t values from the library's own parser (Z = 1), the identity among them.
NP = 300
g1 = []
kk = load()
for i in range(NP):
    buf = C.create_string_buffer(144)
    assert kk.lib.bytes_to_kzg_commitment(buf, cms[i % 3] if i % 7 else b"\xc0" + bytes(47)) == 0
    g1.append(buf.raw)
kk.close()
PTS = b"".join(g1)


def call_sums(k):
    out = C.create_string_buffer(144 * NP)
    ret = k.lib.ckzg_hip_g1_prefix_sums(out, PTS, C.c_uint64(NP), k.sp)
    return ret, out.raw


def want_sums(key, want):
    return None if want[0] == 0 else "%s: unarmed call gave %d" % (key, want[0])


for name, call, want_ok, ret, noun in (("points", call_points, want_points, C_KZG_BADARGS, "verdicts"),
                                       ("blobs", call_blobs, want_blobs, C_KZG_BADARGS, "verdicts"),
                                       ("sums", call_sums, want_sums, 0, "sums")):
    walk(0, (C_KZG_MALLOC,), (0, 1), name + "_allocations", call, want_ok, ret, noun)
    walk(1, (C_KZG_ERROR, C_KZG_MALLOC), (0,), name + "_streams_events", call, want_ok, ret, noun)
print(json.dumps({"report": report, "problems": problems}))
