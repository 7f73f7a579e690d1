"""ckzg_hip_verify_coset_kzg_proof_batch_groups (many coset batches in one call, one verdict per group, coset sizes 2^e,
e = 0 .. 6) against the ways to the same answer that exist without it, at the C-ABI, on valid data in pageable host
memory with the default tables, same box, same process:

    loop        a sequential loop of one ckzg_hip_verify_coset_kzg_proof_batch per group
    one_batch   ONE such call over all items: one verdict for everything -- orientation only
    cell_groups at e = 6 only: ckzg_hip_verify_cell_kzg_proof_batch_groups on the same bytes

    python tools/bench_coset_groups.py [--out profiles/coset_groups_bench.json] [--ab-lib PARENT_BUILD.so] [--runs 20]
                                       [--shapes 128x8,128x64,8x64,512x1] [--es 0,1,2,3,4,5,6]

--ab-lib: a build of the parent commit's library, loaded into the same process; the alternatives are then timed in that
build (the new call exists only in this one).  Without it they are timed in this build.
Per (e, groups x items per group) the variants are alternated, --runs timed repetitions of each after a warm-up round;
median and minimum wall time in milliseconds (every call ends in a device synchronise of its own).  "faster" is claimed
only where the new call's median is below the alternative's minimum; the record says so per row, and says "not faster"
where it is not.  Then one traced call per row (CKZG_HIP_TRACE: the call waits after every stage, so the marks are the
stages' own times and their sum is more than an untraced call).  Prints JSON lines and writes --out."""
import argparse
import ctypes as C
import json
import os
import random
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NAME = "ckzg_hip_verify_coset_kzg_proof_batch_groups"
BLOBS = 4


class Material:
    def __init__(self, hip):
        rnd = random.Random(1)
        self.hip = hip
        self.blobs = [b"".join((rnd.randrange(R)).to_bytes(32, "big") for _ in range(4096)) for _ in range(BLOBS)]
        self.commit = [hip.blob_to_kzg_commitment(b) for b in self.blobs]
        self.level = {}

    def at(self, e):
        if e not in self.level:
            proofs, evals, st = self.hip.compute_coset_kzg_proofs_batch(self.blobs, e, want_evals=True)
            assert st == [0] * BLOBS
            self.level[e] = (proofs, evals)
        return self.level[e]

    def groups(self, e, G, rows):
        """the PeerDAS shape with the coset size a parameter: group g = coset g mod m of `rows` blobs (the base blobs
        repeated), as (commitments, indices, values, proofs) bytes per group"""
        m, per = 8192 >> e, 32 << e
        proofs, evals = self.at(e)
        out = []
        for g in range(G):
            c = g % m
            out.append((b"".join(self.commit[b % BLOBS] for b in range(rows)), [c] * rows,
                        b"".join(evals[b % BLOBS][per * c:per * (c + 1)] for b in range(rows)),
                        b"".join(proofs[b % BLOBS][c] for b in range(rows))))
        return out


def traced(fn, what):
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        os.environ["CKZG_HIP_TRACE"] = "1"
        try:
            fn()
        finally:
            del os.environ["CKZG_HIP_TRACE"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        marks = re.findall(r"\[ckzg-hip trace\] %s: (.*) ([0-9.]+) ms" % what, tmp.read().decode("utf-8", "replace"))
    return {name: float(ms) for name, ms in marks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--shapes", default="128x8,128x64,8x64,512x1")
    ap.add_argument("--es", default="0,1,2,3,4,5,6")
    ap.add_argument("--ab-lib", default="")
    a = ap.parse_args()
    mod = ge.load_package()
    hip = mod.Kzg(mod.HIP_SO)
    old = mod.Kzg(os.path.abspath(a.ab_lib)) if a.ab_lib else hip
    mat = Material(hip)
    groups_fn = getattr(hip.lib, NAME)
    groups_fn.restype = C.c_int
    single = old.lib.ckzg_hip_verify_coset_kzg_proof_batch
    single.restype = C.c_int
    cell_groups = old.lib.ckzg_hip_verify_cell_kzg_proof_batch_groups
    cell_groups.restype = C.c_int
    result = {"tool": "tools/bench_coset_groups.py --runs %d --shapes %s --es %s%s" % (a.runs, a.shapes, a.es, " --ab-lib (the parent commit's build)" if a.ab_lib else ""),
              "stat": "median and min of the wall time over %d timed repetitions per variant, variants alternated, milliseconds; a fresh process, default tables" % a.runs,
              "alternatives_in": "a build of the parent commit, same process" if a.ab_lib else "this build",
              "claim_rule": "faster only where the new call's median is below the alternative's minimum",
              "host_threads": int(hip.lib.ckzg_hip_host_thread_budget()), "cpus_in_affinity_mask": len(os.sched_getaffinity(0)),
              "rows": []}
    for e in (int(v) for v in a.es.split(",")):
        for G, rows in (tuple(int(v) for v in sh.split("x")) for sh in a.shapes.split(",")):
            per_group = mat.groups(e, G, rows)
            n = G * rows
            flat = (b"".join(g[0] for g in per_group), (C.c_uint64 * n)(*[c for g in per_group for c in g[1]]),
                    b"".join(g[2] for g in per_group), b"".join(g[3] for g in per_group))
            one_args = [(g[0], (C.c_uint64 * rows)(*g[1]), g[2], g[3]) for g in per_group]
            start = (C.c_uint64 * (G + 1))(*[rows * g for g in range(G + 1)])
            ok_g, st_g = (C.c_bool * G)(), (C.c_uint8 * G)()

            def v_groups():
                rc = groups_fn(ok_g, st_g, *flat, start, C.c_uint64(G), C.c_uint32(e), hip.sp)
                assert rc == 0 and all(ok_g), (rc, list(ok_g))

            def v_loop():
                okb = C.c_bool(False)
                for args in one_args:
                    rc = single(C.byref(okb), *args, C.c_uint64(rows), C.c_uint32(e), old.sp)
                    assert rc == 0 and okb.value, rc

            def v_one_batch():
                okb = C.c_bool(False)
                rc = single(C.byref(okb), *flat, C.c_uint64(n), C.c_uint32(e), old.sp)
                assert rc == 0 and okb.value, rc

            def v_cell_groups():
                rc = cell_groups(ok_g, st_g, *flat, start, C.c_uint64(G), old.sp)
                assert rc == 0 and all(ok_g), (rc, list(ok_g))

            variants = [("groups", v_groups), ("loop", v_loop), ("one_batch", v_one_batch)]
            if e == 6:
                variants.append(("cell_groups", v_cell_groups))
            for _, fn in variants:   # warm-up: arenas, code objects, the worker pool, the line table of [s^l]_2
                fn()
                fn()
            times = {name: [] for name, _ in variants}
            for _ in range(a.runs):
                for name, fn in variants:
                    t = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - t) * 1e3)
            row = {"e": e, "num_groups": G, "items_per_group": rows}
            for name, _ in variants:
                row[name] = {"median_ms": round(statistics.median(times[name]), 3), "min_ms": round(min(times[name]), 3)}
            for name in ("loop", "cell_groups"):   # the alternatives that give one verdict per group
                if name in row:
                    row["faster_than_" + name] = row["groups"]["median_ms"] < row[name]["min_ms"]
            row["traced_call_stages_ms"] = traced(v_groups, "verify_coset_groups")
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    if old is not hip:
        old.close()
    hip.close()


if __name__ == "__main__":
    main()
