"""Runs under LD_PRELOAD=failalloc.so (tests/test_gpu_coset_openings_alloc.py starts it): every device / page-locked
allocation, then every stream and event creation, of ckzg_hip_compute_coset_kzg_proofs_batch at coset size 16 on fresh
settings -- the lazy transformed setup of that size and the twiddle records included -- is made to fail in turn, once
and (for allocations) from then on.  What must hold each time: the call returns C_KZG_MALLOC (allocations) or
C_KZG_ERROR / C_KZG_MALLOC (streams, events) -- or its normal result, where nothing it needed failed --, never a crash;
no device memory is kept; the same call right after on the same settings builds what the failed one did not keep and
gives the right result.  The batch holds a blob with a non-canonical element between two good ones.  Prints one JSON
line."""
import ctypes as C
import hashlib
import json

from walk import C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC, R, load, problems, report, walk

E = 4
M = 8192 >> E
blobs = [b"".join(b"\x00" + hashlib.sha256(b"cosetwalk%d/%d" % (i, j)).digest()[:31] for j in range(4096)) for i in range(2)]
bad = bytearray(blobs[0])
bad[32 * 9:32 * 10] = R.to_bytes(32, "big")
BLOBS = blobs[0] + bytes(bad) + blobs[1]

# what the good blobs' outputs are, by the call that compute_cells_and_kzg_proofs pins (tests/test_gpu_coset_openings.py
# ties coset size 16 to it): the evaluations are the cells
k0 = load()
CELLS = [b"".join(k0.compute_cells_and_kzg_proofs(b)[0]) for b in blobs]
k0.close()


def call(k):
    proofs, evals, st = C.create_string_buffer(3 * M * 48), C.create_string_buffer(3 * 8192 * 32), (C.c_uint8 * 3)()
    ret = k.lib.ckzg_hip_compute_coset_kzg_proofs_batch(proofs, evals, st, BLOBS, C.c_uint64(3), C.c_uint32(E), k.sp)
    if ret not in (0, C_KZG_BADARGS):
        return (ret,)
    p, ev = proofs.raw, evals.raw
    return ret, p[:M * 48], p[2 * M * 48:], ev[:8192 * 32], ev[2 * 8192 * 32:], bytes(st)


def want_ok(key, want):
    if want[0] != C_KZG_BADARGS or want[5] != bytes([0, 1, 0]) or want[3] != CELLS[0] or want[4] != CELLS[1]:
        return "%s: unarmed call gave %d, statuses %r" % (key, want[0], want[5:])
    if want[1] == bytes(M * 48) or want[1] == want[2]:
        return "%s: unarmed call wrote no proofs" % key
    return None


walk(0, (C_KZG_MALLOC,), (0, 1), "coset_allocations", call, want_ok, C_KZG_BADARGS, "proofs")
walk(1, (C_KZG_ERROR, C_KZG_MALLOC), (0,), "coset_streams_events", call, want_ok, C_KZG_BADARGS, "proofs")
print(json.dumps({"report": report, "problems": problems}))
