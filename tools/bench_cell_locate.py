"""ckzg_hip_verify_cell_kzg_proof_batch_locate (per-cell verdicts at batch cost) against the two existing roads, at the
C-ABI, same box, same session:

  * ckzg_hip_verify_cell_kzg_proof_batch_groups with groups of one (one verdict per cell: the better per-item alternative),
  * one verify_cell_kzg_proof_batch over all cells (ONE verdict for the lot: for scale only).

    python tools/bench_cell_locate.py [--out profiles/cell_locate_bench.json] [--parent-so PATH] [--ab-so PATH] [--runs 20]

--parent-so: a build of the parent commit's library; the two existing calls are then timed in that build (the new call
exists only in this one).  Without it they are timed in this build.
--ab-so: the A/B build of this tree (bash tools/build_variant.sh ab -DCKZG_AB), whose tuning constants are read from the
environment.  With it the tool also records, each in a fresh child process of its own: the window width of the 64-point
table (CKZG_HIP_CELL_LOCATE_WBITS = 8, 10, 12) and the fused one-wave interpolation kernel against the three-pass form
(CKZG_HIP_CELL_INTERP_FUSED = 1, 0), on all-good batches of the two largest sizes; and the first call on a fresh
context, which builds the table.

Per size and number of false cells (0, 1, 8, all): median and minimum wall time over --runs calls and the stats the call
reported.  Also the chunk's leaf hashes alone, on one thread (libhost_shim.so: the same SHA-256 code), for scale against
the call.  Prints one JSON object and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NAME = "ckzg_hip_verify_cell_kzg_proof_batch_locate"


def timed(fn, runs):
    fn()   # warm-up (arena, code objects)
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3)}


def material(hip):
    rnd = random.Random(1)
    out = []
    for _ in range(8):
        blob = b"".join((rnd.randrange(R)).to_bytes(32, "big") for _ in range(4096))
        cells, proofs = hip.compute_cells_and_kzg_proofs(blob)
        out.append((hip.blob_to_kzg_commitment(blob), cells, proofs))
    return out


def case(mat, n, nbad):
    """n cells, column i mod 128 of blob (i / 128) mod 8 (the PeerDAS shape: whole rows); nbad of them (or all) carry
    the proof of the next column"""
    items = []
    for i in range(n):
        b, c = (i // 128) % 8, i % 128
        items.append((mat[b][0], c, mat[b][1][c], mat[b][2][c]))
    bad = set(range(n)) if nbad == "all" else set(random.Random(n).sample(range(n), nbad))
    for i in bad:
        t = items[i]
        items[i] = (t[0], t[1], t[2], mat[(i // 128) % 8][2][(t[1] + 1) % 128])
    exp = [i not in bad for i in range(n)]
    args = (b"".join(t[0] for t in items), (C.c_uint64 * n)(*[t[1] for t in items]), b"".join(t[2] for t in items),
            b"".join(t[3] for t in items))
    return exp, args


def run_locate(hip, n, args, exp, runs):
    f = getattr(hip.lib, NAME)
    f.restype = C.c_int
    ok, st, stats = (C.c_bool * n)(), (C.c_uint8 * n)(), (C.c_uint64 * 3)()

    def call():
        assert f(ok, st, stats, *args, C.c_uint64(n), hip.sp) == 0
    row = timed(call, runs)
    assert list(ok) == exp
    row["stats"] = list(stats)
    return row


def child(a):
    """all-good batches in the library given, tuning constants from the environment: one JSON line"""
    mod = ge.load_package()
    hip = mod.Kzg(os.path.abspath(a.so))
    mat = material(hip)
    out = {"env": {k: v for k, v in os.environ.items() if k.startswith("CKZG_HIP_CELL_")}, "sizes": {}}
    first = True
    for n in [int(x) for x in a.sizes.split(",")]:
        exp, args = case(mat, n, 0)
        if first:
            f = getattr(hip.lib, NAME)
            f.restype = C.c_int
            ok = (C.c_bool * n)()
            t = time.perf_counter()
            assert f(ok, None, None, *args, C.c_uint64(n), hip.sp) == 0
            out["first_call_ms"] = round((time.perf_counter() - t) * 1e3, 3)   # builds the table, grows the arena
            first = False
        out["sizes"][str(n)] = run_locate(hip, n, args, exp, a.runs)
    hip.close()
    print("CHILD " + json.dumps(out), flush=True)


def spawn(a, so, env, sizes):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--so", so, "--sizes", sizes, "--runs", str(a.runs)],
                       env=e, capture_output=True, text=True, timeout=600)
    for line in r.stdout.splitlines():
        if line.startswith("CHILD "):
            return json.loads(line[6:])
    raise SystemExit("bench_cell_locate: child failed (%d)\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-so", default="")
    ap.add_argument("--ab-so", default="")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", default="128,1024,8192,16384")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--so", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    mod = ge.load_package()
    hip = mod.Kzg(mod.HIP_SO)
    old = mod.Kzg(os.path.abspath(a.parent_so)) if a.parent_so else hip
    threads = int(hip.lib.ckzg_hip_host_thread_budget())
    mat = material(hip)
    groups = old.lib.ckzg_hip_verify_cell_kzg_proof_batch_groups
    single = old.lib.verify_cell_kzg_proof_batch
    groups.restype = single.restype = C.c_int
    sizes = [int(x) for x in a.sizes.split(",")]
    res = {"tool": "bench_cell_locate", "host_threads": threads, "cpus_in_affinity_mask": len(os.sched_getaffinity(0)), "runs": a.runs,
           "existing_calls_timed_in": "parent build" if a.parent_so else "this build", "cells": []}
    for n in sizes:
        exp, args = case(mat, n, 0)
        start = (C.c_uint64 * (n + 1))(*range(n + 1))
        ok2, st2, one = (C.c_bool * n)(), (C.c_uint8 * n)(), C.c_bool(False)
        row = {"n": n,
               "groups_of_one": timed(lambda: groups(ok2, st2, *args, start, C.c_uint64(n), old.sp), a.runs),
               "one_batch_one_verdict": timed(lambda: single(C.byref(one), *args, C.c_uint64(n), old.sp), a.runs), "locate": {}}
        assert all(ok2) and one.value
        for nbad in (0, 1, 8, "all"):
            exp, args = case(mat, n, nbad)
            row["locate"][str(nbad)] = run_locate(hip, n, args, exp, a.runs)
        row["claim_holds"] = row["locate"]["0"]["median_ms"] < row["groups_of_one"]["min_ms"]
        res["cells"].append(row)
        print(json.dumps(row), flush=True)

    # ---- the leaf hashes of the largest chunk alone, on one thread ----
    shim = os.path.join(ROOT, "c-kzg-4844_amd", "csrc", "libhost_shim.so")
    if os.path.exists(shim):
        h = C.CDLL(shim)
        h.hs_locate_cell_digest.restype = None
        n = max(sizes)
        _, args = case(mat, n, 0)
        out = C.create_string_buffer(32)
        t = timed(lambda: h.hs_locate_cell_digest(out, *args, C.c_uint64(n)), 5)
        res["leaf_hashes"] = {"n": n, "one_thread": t, "pool_threads": min(threads, 32),
                              "one_thread_median_over_pool_threads_ms": round(t["median_ms"] / max(1, min(threads, 32)), 3)}
        print(json.dumps(res["leaf_hashes"]), flush=True)

    # ---- table width and the form of the interpolation, each in a child process of the A/B build ----
    if a.ab_so:
        big = ",".join(str(n) for n in sizes[-2:])
        res["table_wbits_sweep"] = [spawn(a, a.ab_so, {"CKZG_HIP_CELL_LOCATE_WBITS": str(w), "CKZG_HIP_CELL_INTERP_FUSED": "1"}, big)
                                    for w in (8, 10, 12)]
        print(json.dumps(res["table_wbits_sweep"]), flush=True)
        res["interp_fused_vs_three_pass"] = [spawn(a, a.ab_so, {"CKZG_HIP_CELL_LOCATE_WBITS": "8", "CKZG_HIP_CELL_INTERP_FUSED": str(f)}, big)
                                             for f in (1, 0, 1, 0)]
        print(json.dumps(res["interp_fused_vs_three_pass"]), flush=True)

    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    hip.close()
    if old is not hip:
        old.close()


if __name__ == "__main__":
    main()
