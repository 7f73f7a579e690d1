"""Runs under LD_PRELOAD=failalloc.so (tests/test_point_openings_alloc.py starts it): every device / page-locked
allocation, then every stream and event creation, of ckzg_hip_compute_kzg_proof_batch and of its _device form is made to
fail in turn, once and (for allocations) from then on.  What must hold each time: the call returns C_KZG_MALLOC
(allocations) or C_KZG_ERROR / C_KZG_MALLOC (streams, events) -- or its normal result, where nothing it needed failed
--, never a crash; no device memory is kept; the same call right after on the same settings gives the right results.
The batch spans two chunks of the call, mixes domain-point and random z and holds one invalid item.  The device form's
own buffers are allocated before any failure is armed.  Prints one JSON line."""
import ctypes as C
import json
import random

from walk import C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC, R, fr, load, problems, report, walk

rt = C.CDLL("/opt/rocm/lib/libamdhip64.so")
rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
CHUNK = 256   # ckzg_api2.hip: POINT_CHUNK
BLOB = 131072

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

for form, call_raw, want_ret in (("host", call_host, C_KZG_BADARGS), ("device", call_device, 0)):
    def call(k, call_raw=call_raw):
        return valid_part(call_raw(k))

    def want_ok(key, want, want_ret=want_ret):
        if want[0] != want_ret or want[1].count(C_KZG_BADARGS) != 1:
            return "%s: unarmed call gave %d with %d invalid items" % (key, want[0], want[1].count(C_KZG_BADARGS))
        return None

    walk(0, (C_KZG_MALLOC,), (0, 1), form + "_allocations", call, want_ok, want_ret, "results")
    walk(1, (C_KZG_ERROR, C_KZG_MALLOC), (0,), form + "_streams_events", call, want_ok, want_ret, "results")
print(json.dumps({"report": report, "problems": problems}))
