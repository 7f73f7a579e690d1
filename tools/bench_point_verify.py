"""ckzg_hip_verify_kzg_proof_batch (one verify_kzg_proof per item, pairings on the GPU) against a loop of the
single-item verify_kzg_proof on ckzg_hip_host_thread_budget() host threads (ctypes releases the GIL), at the C-ABI.

    python tools/bench_point_verify.py [--out FILE] [--sizes 1,64,...] [--gpu-only]

Prints one JSON object (and writes it to FILE): per n the best wall time of the batch call over a few repetitions,
the host loop's best wall time and the ratio (every size measured, none extrapolated), plus the smallest measured n from
which on the batch call is faster at every larger measured size.  --gpu-only
skips the host loop (for a `rocprofv3 --kernel-trace --stats` run of its own, which gives the device time of
k_point_lhs and k_pairing_check)."""
import argparse
import ctypes as C
import json
import os
import random
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def fr(v):
    return (v % R).to_bytes(32, "big")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="1,16,64,128,256,512,768,1024,1280,1536,2048,2560,3072,4096,65536")
    ap.add_argument("--gpu-only", action="store_true")
    a = ap.parse_args()
    mod = ge.load_package()
    hip = mod.Kzg(mod.HIP_SO)
    rnd = random.Random(1)
    tuples = []
    for i in range(16):
        blob = b"".join(fr(rnd.randrange(R)) for _ in range(4096))
        c = hip.blob_to_kzg_commitment(blob)
        z = fr(rnd.randrange(R))
        p, y = hip.compute_kzg_proof(blob, z)
        tuples.append((c, z, y, p))
    f = hip.lib.ckzg_hip_verify_kzg_proof_batch
    f.restype = C.c_int
    single = hip.lib.verify_kzg_proof
    single.restype = C.c_int
    threads = int(hip.lib.ckzg_hip_host_thread_budget())
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        items = [tuples[i % len(tuples)] for i in range(n)]
        cc, zz, yy, pp = (b"".join(t[k] for t in items) for k in range(4))
        ok = (C.c_bool * n)()
        st = (C.c_uint8 * n)()
        rc = f(ok, st, cc, zz, yy, pp, C.c_uint64(n), hip.sp)   # warm-up (arena, code object)
        assert rc == 0 and all(ok), rc
        best = 1e9
        for _ in range(2 if n >= 65536 else 4):
            t = time.perf_counter()
            rc = f(ok, st, cc, zz, yy, pp, C.c_uint64(n), hip.sp)
            best = min(best, time.perf_counter() - t)
        row = {"n": n, "gpu_ms": round(best * 1e3, 3)}
        if not a.gpu_only:
            def work(nxt, lock):
                okb = C.c_bool(False)
                while True:
                    with lock:
                        i = nxt[0]
                        nxt[0] += 1
                    if i >= n:
                        return
                    c, z, y, p = items[i]
                    single(C.byref(okb), c, z, y, p, hip.sp)

            host = 1e9
            for _ in range(3 if n <= 4096 else 1):   # best of three: one loop is noisy at a few ms
                nxt, lock = [0], threading.Lock()
                t = time.perf_counter()
                th = [threading.Thread(target=work, args=(nxt, lock)) for _ in range(min(threads, n))]
                for x in th:
                    x.start()
                for x in th:
                    x.join()
                host = min(host, time.perf_counter() - t)
            row.update({"host_loop_ms": round(host * 1e3, 3), "host_over_gpu": round(host / best, 2)})
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "bench_point_verify", "host_threads": threads, "cpus_in_affinity_mask": len(os.sched_getaffinity(0)),
           "rows": rows}
    if not a.gpu_only:
        cross = None
        for r in reversed(rows):   # the smallest measured n from which on the batch call wins at every larger size
            if r["host_loop_ms"] <= r["gpu_ms"]:
                break
            cross = r["n"]
        res["crossover_n"] = cross
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    hip.close()


if __name__ == "__main__":
    main()
