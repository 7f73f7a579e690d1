"""ckzg_hip_verify_blob_kzg_proof_batch_groups (many blob batches in one call, one verdict per group) against the ways
of getting per-group verdicts from verify_blob_kzg_proof_batch, at the C-ABI, on valid data in pageable host memory
with the default tables.  The shapes: a transaction pool's blob transactions (128 x 6, 8 x 6), a range of blocks at
the blob limit (64 x 9), single-blob transactions (512 x 1).

    python tools/bench_blob_groups.py [--out FILE] [--reps 20] [--shapes 128x6,64x9,8x6,512x1]
                                      [--lib OTHER_BUILD.so] [--parent FILE]

Per shape (groups x blobs per group) the variants are alternated in one process, `--reps` timed repetitions of each
after a warm-up round; median and min in milliseconds:
    groups_call  (a) the new call
    loop         (b) a sequential loop of one verify_blob_kzg_proof_batch per group
    threads16    (c) 16 host threads sharing those calls (ctypes releases the GIL)
    one_batch    (d) ONE verify_blob_kzg_proof_batch over all blobs: one verdict for everything -- orientation only
Then one traced call of (a) per shape (CKZG_HIP_TRACE: the call waits after every stage, so the marks are the stages'
own times, and their sum is more than an untraced call).
--lib times (b), (c) and (d) only, on another build of the library (the parent commit's).  --parent FILE takes the JSON
such a run wrote, embeds it and judges per shape: the median of (a) below the minimum over repetitions of the better
of the parent build's (b) and (c).  Prints one JSON object and writes it to FILE."""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def clocks():
    """the box's GPU clocks as rocm-smi reports them (read only), or why they are not known"""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else {"unavailable": r.stderr.strip()[-200:]}
    except Exception as e:   # no rocm-smi, no permission, no JSON: the timings stand without it
        return {"unavailable": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="128x6,64x9,8x6,512x1")
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent", default="")
    a = ap.parse_args()
    mod = ge.load_package()
    hip = mod.Kzg(os.path.abspath(a.lib) if a.lib else mod.HIP_SO)
    mat = []
    for i in range(8):
        blob = b"".join(b"\x00" + hashlib.sha256(b"bench%d/%d" % (i, j)).digest()[:31] for j in range(4096))
        cm = hip.blob_to_kzg_commitment(blob)
        mat.append((blob, cm, hip.compute_blob_kzg_proof(blob, cm)))
    single = hip.lib.verify_blob_kzg_proof_batch
    single.restype = C.c_int
    groups_fn = None
    if not a.lib:
        groups_fn = hip.lib.ckzg_hip_verify_blob_kzg_proof_batch_groups
        groups_fn.restype = C.c_int
    result = {"tool": "tools/bench_blob_groups.py --reps %d --shapes %s%s" % (a.reps, a.shapes, " --lib (another build)" if a.lib else ""),
              "stat": "median and min over %d timed repetitions per variant, variants alternated, milliseconds" % a.reps,
              "host_threads": int(hip.lib.ckzg_hip_host_thread_budget()), "cpus_in_affinity_mask": len(os.sched_getaffinity(0)),
              "clocks_before": clocks(), "shapes": []}
    for G, per in (tuple(int(v) for v in sh.split("x")) for sh in a.shapes.split(",")):
        per_group = []
        for g in range(G):
            ids = [(g + i) % 8 for i in range(per)]
            per_group.append(tuple(b"".join(mat[b][k] for b in ids) for k in range(3)))
        n = G * per
        flat = tuple(b"".join(g[k] for g in per_group) for k in range(3))
        start = (C.c_uint64 * (G + 1))(*[per * g for g in range(G + 1)])
        ok_g, st_g = (C.c_bool * G)(), (C.c_uint8 * G)()

        def v_groups():
            rc = groups_fn(ok_g, st_g, flat[0], flat[1], flat[2], start, C.c_uint64(G), hip.sp)
            assert rc == 0 and all(ok_g), (rc, list(ok_g))

        def one(g, okb):
            bl, cm, pr = per_group[g]
            rc = single(C.byref(okb), bl, cm, pr, C.c_uint64(per), hip.sp)
            assert rc == 0 and okb.value, (g, rc)

        def v_loop():
            okb = C.c_bool(False)
            for g in range(G):
                one(g, okb)

        def v_threads():
            nxt, lock, errs = [0], threading.Lock(), []

            def work():
                okb = C.c_bool(False)
                try:
                    while True:
                        with lock:
                            g = nxt[0]
                            nxt[0] += 1
                        if g >= G:
                            return
                        one(g, okb)
                except AssertionError as e:
                    errs.append(e)

            th = [threading.Thread(target=work) for _ in range(16)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            assert not errs, errs[:1]

        def v_one_batch():
            okb = C.c_bool(False)
            rc = single(C.byref(okb), flat[0], flat[1], flat[2], C.c_uint64(n), hip.sp)
            assert rc == 0 and okb.value, rc

        variants = [("groups_call", v_groups)] if groups_fn else []
        variants += [("loop", v_loop), ("threads16", v_threads), ("one_batch", v_one_batch)]
        for _, fn in variants:   # warm-up: arenas, code objects, the worker pool
            fn()
            fn()
        times = {name: [] for name, _ in variants}
        for _ in range(a.reps):
            for name, fn in variants:
                t = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t) * 1e3)
        row = {"num_groups": G, "blobs_per_group": per}
        for name, _ in variants:
            row[name] = {"median_ms": round(statistics.median(times[name]), 3), "min_ms": round(min(times[name]), 3)}
        if groups_fn:
            # one traced call: the stages of the new call
            with tempfile.TemporaryFile() as tmp:
                sys.stderr.flush()
                saved = os.dup(2)
                os.dup2(tmp.fileno(), 2)
                os.environ["CKZG_HIP_TRACE"] = "1"
                try:
                    v_groups()
                finally:
                    del os.environ["CKZG_HIP_TRACE"]
                    os.dup2(saved, 2)
                    os.close(saved)
                tmp.seek(0)
                marks = re.findall(r"\[ckzg-hip trace\] verify_blob_groups: (.*) ([0-9.]+) ms", tmp.read().decode("utf-8", "replace"))
            row["traced_call_stages_ms"] = {name: float(ms) for name, ms in marks}
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    result["clocks_after"] = clocks()
    if a.parent and groups_fn:
        with open(a.parent) as fh:
            parent = json.load(fh)
        result["parent_build"] = parent
        by_shape = {(r["num_groups"], r["blobs_per_group"]): r for r in parent["shapes"]}
        for row in result["shapes"]:
            p = by_shape.get((row["num_groups"], row["blobs_per_group"]))
            if p:
                best = min(p["loop"]["min_ms"], p["threads16"]["min_ms"])
                row["criterion"] = {"groups_call_median_ms": row["groups_call"]["median_ms"],
                                    "parent_best_of_loop_threads16_min_ms": best,
                                    "met": row["groups_call"]["median_ms"] < best}
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    hip.close()


if __name__ == "__main__":
    main()
