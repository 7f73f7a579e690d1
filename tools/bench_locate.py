"""ckzg_hip_verify_kzg_proof_batch_locate / ckzg_hip_verify_blob_kzg_proof_batch_locate (per-item verdicts at batch
cost: prefix sums on the GPU, bisection on the host pool) against the three existing roads to a verdict per item, at
the C-ABI, same box, same session:

  * ckzg_hip_verify_kzg_proof_batch (one two-pairing check per item on a GPU lane),
  * a loop of verify_kzg_proof on ckzg_hip_host_thread_budget() host threads (ctypes releases the GIL),
  * for blobs, ckzg_hip_verify_blob_kzg_proof_batch_groups with groups of one.

    python tools/bench_locate.py [--out profiles/locate_bench.json] [--parent-so PATH] [--runs 20]

--parent-so: a build of the parent commit's library; the three existing calls are then timed in that build (the new
calls exist only in this one).  Without it they are timed in this build.  Per size and number of false items: median
and minimum wall time over --runs calls (the host loop: 3 runs up to 512 items, 1 above), and the stats the call
reported.  Also measures the two rates that set the default of the option "locate_max_checks" -- the host pool's range
checks per millisecond (a bisection of an all-false chunk of 1,024 items, no hand-over, minus the same call on an
all-good chunk) and the per-lane pass over a full chunk
(hand-over at the root of an all-false chunk, minus the same call on an all-good chunk) -- and their product rounded
down to a power of two.  Prints one JSON object and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
UNLIMITED = 1 << 40


def fr(v):
    return (v % R).to_bytes(32, "big")


def timed(fn, runs):
    fn()   # warm-up (arena, code objects)
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3)}


def host_loop(single, sp, calls, threads, runs):
    """calls: one tuple of byte strings per item"""
    n = len(calls)

    def work(nxt, lock):
        okb = C.c_bool(False)
        while True:
            with lock:
                i = nxt[0]
                nxt[0] += 1
            if i >= n:
                return
            single(C.byref(okb), *calls[i], sp)

    ts = []
    for _ in range(runs):
        nxt, lock = [0], threading.Lock()
        t = time.perf_counter()
        th = [threading.Thread(target=work, args=(nxt, lock)) for _ in range(min(threads, n))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-so", default="")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", default="64,512,4096,65536")
    ap.add_argument("--blob-sizes", default="8,64,512")
    a = ap.parse_args()
    mod = ge.load_package()
    hip = mod.Kzg(mod.HIP_SO)
    old = mod.Kzg(os.path.abspath(a.parent_so)) if a.parent_so else hip
    setopt = hip.lib.ckzg_hip_set_option
    setopt.restype = C.c_int
    setopt.argtypes = [C.c_char_p, C.c_int64]
    threads = int(hip.lib.ckzg_hip_host_thread_budget())
    rnd = random.Random(1)
    blobs, tuples = [], []
    for i in range(16):
        blob = b"".join(fr(rnd.randrange(R)) for _ in range(4096))
        c = hip.blob_to_kzg_commitment(blob)
        z = fr(rnd.randrange(R))
        p, y = hip.compute_kzg_proof(blob, z)
        tuples.append((c, z, y, p))
        blobs.append((blob, c, hip.compute_blob_kzg_proof(blob, c)))
    wrong = lambda t: (t[0], t[1], fr(int.from_bytes(t[2], "big") + 1), t[3])
    locate = hip.lib.ckzg_hip_verify_kzg_proof_batch_locate
    per_item = old.lib.ckzg_hip_verify_kzg_proof_batch
    single = old.lib.verify_kzg_proof
    for f in (locate, per_item, single):
        f.restype = C.c_int

    def point_case(n, nbad):
        items = [tuples[i % 16] for i in range(n)]
        for i in (range(n) if nbad == "all" else random.Random(n).sample(range(n), nbad)):
            items[i] = wrong(items[i])
        exp = [it in tuples for it in items]
        return items, exp, tuple(b"".join(t[k] for t in items) for k in range(4))

    def run_locate(n, args, exp):
        ok, st, stats = (C.c_bool * n)(), (C.c_uint8 * n)(), (C.c_uint64 * 3)()

        def call():
            assert locate(ok, st, stats, *args, C.c_uint64(n), hip.sp) == 0
        row = timed(call, a.runs)
        assert list(ok) == exp
        row["stats"] = list(stats)
        return row

    res = {"tool": "bench_locate", "host_threads": threads, "cpus_in_affinity_mask": len(os.sched_getaffinity(0)), "runs": a.runs,
           "existing_calls_timed_in": "parent build" if a.parent_so else "this build", "points": [], "blobs": []}

    # ---- the two rates behind the default of locate_max_checks ----
    assert setopt(b"locate_max_checks", UNLIMITED) == 0
    n = 1024
    _, exp, args = point_case(n, "all")
    bis = run_locate(n, args, exp)
    _, exp_good, args_good = point_case(n, 0)
    good = run_locate(n, args_good, exp_good)
    checks_per_ms = (bis["stats"][0] - 1) / (bis["median_ms"] - good["median_ms"])
    n = 65536
    _, exp, args = point_case(n, "all")
    assert setopt(b"locate_max_checks", 0) == 0
    lane = run_locate(n, args, exp)
    _, exp_good, args_good = point_case(n, 0)
    good = run_locate(n, args_good, exp_good)
    lane_ms = lane["median_ms"] - good["median_ms"]
    crossover = checks_per_ms * lane_ms
    default = 1
    while default * 2 <= crossover:
        default *= 2
    res["locate_max_checks"] = {"host_range_checks_per_ms": round(checks_per_ms, 2), "per_lane_pass_ms_65536": round(lane_ms, 3),
                                "crossover_checks": round(crossover, 1), "default": default}
    print(json.dumps(res["locate_max_checks"]), flush=True)
    assert setopt(b"locate_max_checks", default) == 0

    # ---- point form ----
    for n in [int(x) for x in a.sizes.split(",")]:
        items, exp, args = point_case(n, 0)
        ok, st = (C.c_bool * n)(), (C.c_uint8 * n)()
        row = {"n": n, "per_item_gpu": timed(lambda: per_item(ok, st, *args, C.c_uint64(n), old.sp), a.runs),
               "host_loop": host_loop(single, old.sp, items, threads, 3 if n <= 512 else 1), "locate": {}}
        for nbad in (0, 1, 8, "all"):
            if nbad != "all" and nbad > n:
                continue
            _, exp, args = point_case(n, nbad)
            row["locate"][str(nbad)] = run_locate(n, args, exp)
        res["points"].append(row)
        print(json.dumps(row), flush=True)

    # ---- blob form ----
    blocate = hip.lib.ckzg_hip_verify_blob_kzg_proof_batch_locate
    groups = old.lib.ckzg_hip_verify_blob_kzg_proof_batch_groups
    for f in (blocate, groups):
        f.restype = C.c_int
    for n in [int(x) for x in a.blob_sizes.split(",")]:
        row = {"n": n, "locate": {}}
        for nbad in (0, 1, 8, "all"):
            items = [blobs[i % 16] for i in range(n)]
            for i in (range(n) if nbad == "all" else random.Random(n).sample(range(n), nbad)):
                items[i] = (items[i][0], items[i][1], blobs[(i + 1) % 16][2])   # another blob's proof
            exp = [it in blobs for it in items]
            bb, cc, pp = (b"".join(t[k] for t in items) for k in range(3))
            ok, st, stats = (C.c_bool * n)(), (C.c_uint8 * n)(), (C.c_uint64 * 3)()

            def call():
                assert blocate(ok, st, stats, bb, cc, pp, C.c_uint64(n), hip.sp) == 0
            r = timed(call, a.runs)
            assert list(ok) == exp
            r["stats"] = list(stats)
            row["locate"][str(nbad)] = r
            if nbad == 0:
                start = (C.c_uint64 * (n + 1))(*range(n + 1))
                ok2, st2 = (C.c_bool * n)(), (C.c_uint8 * n)()
                row["groups_of_one"] = timed(lambda: groups(ok2, st2, bb, cc, pp, start, C.c_uint64(n), old.sp), a.runs)
                assert all(ok2)
        res["blobs"].append(row)
        print(json.dumps(row), flush=True)

    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    hip.close()
    if old is not hip:
        old.close()


if __name__ == "__main__":
    main()
