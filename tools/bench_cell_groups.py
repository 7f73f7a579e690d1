"""ckzg_hip_verify_cell_kzg_proof_batch_groups (many cell batches in one call, one verdict per group) against the ways
of getting per-group verdicts from verify_cell_kzg_proof_batch, at the C-ABI, on valid data in pageable host memory
with the default tables.  The PeerDAS shape: group c = column c of every blob of a block.

    python tools/bench_cell_groups.py [--out FILE] [--reps 20] [--shapes 128x64,8x64,128x8] [--lib OTHER_BUILD.so]
                                      [--ab-lib PARENT_BUILD.so]

Per shape (groups x cells per group) the variants are alternated in one process, `--reps` timed repetitions of each
after a warm-up round; median and min in milliseconds:
    groups       (a) the new call
    loop         (b) a sequential loop of one verify_cell_kzg_proof_batch per group
    threads16    (c) 16 host threads sharing those calls (ctypes releases the GIL)
    one_batch    (d) ONE verify_cell_kzg_proof_batch over all cells: one verdict for everything -- orientation only
128 x 64 gets all four, every other shape (a) and (b).  Then one traced call of (a) per shape (CKZG_HIP_TRACE: the
call waits after every stage, so the marks are the stages' own times, and their sum is more than an untraced call).
--lib times (b) and (d) only, on another build of the library (the parent commit's: both variants go through code this
call does not touch, so the two builds should agree).  --ab-lib adds the variant groups_ab: (a) in another build of the
library (the parent commit's), loaded into the same process and alternated with the others (block medians of both builds
with the parent's own spread as the margin: tools/bench_groups_merge_ab.py).  Prints one JSON object and writes it to
FILE."""
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
    ap.add_argument("--shapes", default="128x64,8x64,128x8")
    ap.add_argument("--lib", default="")
    ap.add_argument("--ab-lib", default="")
    a = ap.parse_args()
    mod = ge.load_package()
    hip = mod.Kzg(os.path.abspath(a.lib) if a.lib else mod.HIP_SO)
    ab = mod.Kzg(os.path.abspath(a.ab_lib)) if a.ab_lib else None
    groups_ab = None
    if ab:
        groups_ab = ab.lib.ckzg_hip_verify_cell_kzg_proof_batch_groups
        groups_ab.restype = C.c_int
    mat = []
    for i in range(8):
        blob = b"".join(b"\x00" + hashlib.sha256(b"bench%d/%d" % (i, j)).digest()[:31] for j in range(4096))
        cells, proofs = hip.compute_cells_and_kzg_proofs(blob)
        mat.append((hip.blob_to_kzg_commitment(blob), cells, proofs))
    single = hip.lib.verify_cell_kzg_proof_batch
    single.restype = C.c_int
    groups_fn = None
    if not a.lib:
        groups_fn = hip.lib.ckzg_hip_verify_cell_kzg_proof_batch_groups
        groups_fn.restype = C.c_int
    result = {"tool": "tools/bench_cell_groups.py --reps %d --shapes %s%s" % (a.reps, a.shapes, " --lib (another build)" if a.lib else ""),
              "stat": "median and min over %d timed repetitions per variant, variants alternated, milliseconds" % a.reps,
              "host_threads": int(hip.lib.ckzg_hip_host_thread_budget()), "cpus_in_affinity_mask": len(os.sched_getaffinity(0)),
              "clocks_before": clocks(), "shapes": []}
    for G, rows in (tuple(int(v) for v in sh.split("x")) for sh in a.shapes.split(",")):
        full = (G, rows) == (128, 64)
        per_group = []
        for g in range(G):
            c = g % 128
            cm = b"".join(mat[b % 8][0] for b in range(rows))
            idx = (C.c_uint64 * rows)(*([c] * rows))
            cl = b"".join(mat[b % 8][1][c] for b in range(rows))
            pr = b"".join(mat[b % 8][2][c] for b in range(rows))
            per_group.append((cm, idx, cl, pr))
        n = G * rows
        flat = (b"".join(g[0] for g in per_group), (C.c_uint64 * n)(*[g % 128 for g in range(G) for _ in range(rows)]),
                b"".join(g[2] for g in per_group), b"".join(g[3] for g in per_group))
        start = (C.c_uint64 * (G + 1))(*[rows * g for g in range(G + 1)])
        ok_g, st_g = (C.c_bool * G)(), (C.c_uint8 * G)()

        def v_groups(f=groups_fn, api=hip):
            rc = f(ok_g, st_g, flat[0], flat[1], flat[2], flat[3], start, C.c_uint64(G), api.sp)
            assert rc == 0 and all(ok_g), (rc, list(ok_g))

        def one(g, okb):
            cm, idx, cl, pr = per_group[g]
            rc = single(C.byref(okb), cm, idx, cl, pr, C.c_uint64(rows), hip.sp)
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
            rc = single(C.byref(okb), flat[0], flat[1], flat[2], flat[3], C.c_uint64(n), hip.sp)
            assert rc == 0 and okb.value, rc

        variants = []
        if groups_fn:
            variants.append(("groups", v_groups))
        if groups_ab:
            variants.append(("groups_ab", lambda: v_groups(groups_ab, ab)))
        variants.append(("loop", v_loop))
        if full and groups_fn:
            variants.append(("threads16", v_threads))
        if full:
            variants.append(("one_batch", v_one_batch))
        for _, fn in variants:   # warm-up: arenas, code objects, the worker pool
            fn()
            fn()
        times = {name: [] for name, _ in variants}
        for _ in range(a.reps):
            for name, fn in variants:
                t = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t) * 1e3)
        row = {"groups": G, "cells_per_group": rows}
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
                marks = re.findall(r"\[ckzg-hip trace\] verify_cell_groups: (.*) ([0-9.]+) ms", tmp.read().decode("utf-8", "replace"))
            row["traced_call_stages_ms"] = {name: float(ms) for name, ms in marks}
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    result["clocks_after"] = clocks()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    if ab:
        ab.close()
    hip.close()


if __name__ == "__main__":
    main()
