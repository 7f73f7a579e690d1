"""ckzg_hip_compute_kzg_proof_batch (compute_kzg_proof over n (blob, z) items, every item on the GPU) at the C-ABI:
the batch at n = 1, 64, 1024, 4096 with all-random z and with all-domain-point z, the single compute_kzg_proof at a
domain point and at a random z, and ckzg_hip_compute_blob_kzg_proof_batch at 1024 (the path that lost its host fallback
for challenges on the domain).

    python tools/bench_point_openings.py [--out FILE] [--sizes 1,64,1024,4096] [--reps K]

Every row is the median wall time of K timed calls after one warm-up call.  Prints one JSON object (and writes it to
FILE).  Against another build of the library (CKZG_HIP_SO=path, e.g. the parent commit's) the rows whose entry point
that build lacks are left out; the single calls and the blob-proof batch are measured on any build."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def fr(v):
    return (v % R).to_bytes(32, "big")


def brp(i, bits=12):
    return int(format(i, "0%db" % bits)[::-1], 2)


def timed(fn, reps):
    fn()   # warm-up (arena, code objects)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return round(statistics.median(t) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="1,64,1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    mod = ge.load_package()
    hip = mod.Kzg(mod.HIP_SO)
    rnd = random.Random(1)
    blobs = [b"".join(fr(rnd.randrange(R)) for _ in range(4096)) for _ in range(16)]
    w = pow(7, (R - 1) // 4096, R)
    res = {"tool": "bench_point_openings", "lib": os.path.basename(os.path.dirname(os.path.abspath(mod.HIP_SO))),
           "reps": a.reps, "stat": "median_ms"}
    proof, y = C.create_string_buffer(48), C.create_string_buffer(32)
    single = hip.lib.compute_kzg_proof
    single.restype = C.c_int
    for name, z in (("single_domain_ms", fr(pow(w, brp(1234), R))), ("single_random_ms", fr(rnd.randrange(R)))):
        def one(z=z):
            assert single(proof, y, blobs[0], z, hip.sp) == 0
        res[name] = timed(one, max(a.reps, 21))
    if hasattr(hip.lib, "ckzg_hip_compute_kzg_proof_batch"):
        f = hip.lib.ckzg_hip_compute_kzg_proof_batch
        f.restype = C.c_int
        rows = []
        for n in [int(x) for x in a.sizes.split(",")]:
            bb = b"".join(blobs[i % len(blobs)] for i in range(n))
            zr = b"".join(fr(rnd.randrange(R)) for _ in range(n))
            zd = b"".join(fr(pow(w, brp(rnd.randrange(4096)), R)) for _ in range(n))
            pr, ys, st = C.create_string_buffer(48 * n), C.create_string_buffer(32 * n), (C.c_uint8 * n)()
            row = {"n": n}
            for key, zz in (("random_z_ms", zr), ("domain_z_ms", zd)):
                def call(zz=zz):
                    assert f(pr, ys, st, bb, zz, C.c_uint64(n), hip.sp) == 0
                row[key] = timed(call, a.reps if n < 4096 else max(3, a.reps // 2))
            row["domain_over_random"] = round(row["domain_z_ms"] / row["random_z_ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
        res["batch"] = rows
    n = 1024
    bb = b"".join(blobs[i % len(blobs)] for i in range(n))
    cms = [hip.blob_to_kzg_commitment(b) for b in blobs]
    cc = b"".join(cms[i % len(blobs)] for i in range(n))
    g = hip.lib.ckzg_hip_compute_blob_kzg_proof_batch
    g.restype = C.c_int
    pr, st = C.create_string_buffer(48 * n), (C.c_uint8 * n)()

    def blob_batch():
        assert g(pr, st, bb, cc, C.c_uint64(n), hip.sp) == 0
    res["blob_proof_batch_1024_ms"] = timed(blob_batch, a.reps)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    hip.close()


if __name__ == "__main__":
    main()
