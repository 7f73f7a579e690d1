"""ckzg_hip_verify_blob_cell_kzg_proof_batch_groups (blobs against their 128 cell proofs each, one verdict per group)
against what a client has to write without it, at the C-ABI, on valid data in pageable host memory with the default
tables.  The shape of a transaction pool: a group is one blob transaction.

    python tools/bench_blob_cell_groups.py [--out FILE] [--reps 20] [--shapes 128x6,8x6,64x1,1x6,1x1]
                                           [--parent-lib PARENT_BUILD.so] [--ab-lib AB_BUILD.so]

Per shape (groups x blobs per group) the variants are alternated in one process (the order rotated from one repetition
to the next), `--reps` timed repetitions of each after a warm-up round; median and min in milliseconds:
    new          (a) the new call
    composed     (b) ckzg_hip_compute_cells_and_kzg_proofs_batch (cells only) over all blobs, the repeated commitment and
                     index arrays built on the host, then ckzg_hip_verify_cell_kzg_proof_batch_groups; one thread
    loop         (c) per group: compute_cells_and_kzg_proofs (cells only) per blob, then one verify_cell_kzg_proof_batch:
                     the reference API's shape
(b) and (c) run on --parent-lib (a build of the parent commit: tools/build_variant.sh, or the parent's own
libckzg_hip.so) with settings of its own in the same process; without it they run on the product and the record says so.
--ab-lib (a -DCKZG_AB build of THIS commit) adds, for shapes of one group, the two routes such a call can take:
    new_chunk    the chunk path with G = 1
    new_staged   cells staged in page-locked memory, then the single-batch path
Criterion, per shape: median of (a) below the minimum of the better of (b) and (c).  Then one traced call of (a) per
shape (CKZG_HIP_TRACE: the call waits after every stage, so the marks are the stages' own times, and their sum is more
than an untraced call).  Prints one JSON object and writes it to FILE."""
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
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

NEW = "ckzg_hip_verify_blob_cell_kzg_proof_batch_groups"
KNOB = "CKZG_HIP_BLOB_CELL_ONE_STAGED"


def clocks():
    """the box's GPU clocks as rocm-smi reports them (read only), or why they are not known"""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else {"unavailable": r.stderr.strip()[-200:]}
    except Exception as e:   # no rocm-smi, no permission, no JSON: the timings stand without it
        return {"unavailable": repr(e)}


def fn(api, name):
    f = getattr(api.lib, name)
    f.restype = C.c_int
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="128x6,8x6,64x1,1x6,1x1")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--ab-lib", default="")
    a = ap.parse_args()
    mod = ge.load_package()
    hip = mod.Kzg(mod.HIP_SO)
    old = mod.Kzg(os.path.abspath(a.parent_lib)) if a.parent_lib else hip
    ab = mod.Kzg(os.path.abspath(a.ab_lib)) if a.ab_lib else None
    mat = []
    for i in range(4):
        blob = b"".join(b"\x00" + hashlib.sha256(b"bench%d/%d" % (i, j)).digest()[:31] for j in range(4096))
        _, proofs = hip.compute_cells_and_kzg_proofs(blob)
        mat.append((blob, hip.blob_to_kzg_commitment(blob), b"".join(proofs)))
    new_fn = fn(hip, NEW)
    new_ab = fn(ab, NEW) if ab else None
    cells_batch = fn(old, "ckzg_hip_compute_cells_and_kzg_proofs_batch")
    cell_groups = fn(old, "ckzg_hip_verify_cell_kzg_proof_batch_groups")
    cells_one = fn(old, "compute_cells_and_kzg_proofs")
    verify_one = fn(old, "verify_cell_kzg_proof_batch")
    result = {"tool": "tools/bench_blob_cell_groups.py --reps %d --shapes %s" % (a.reps, a.shapes),
              "stat": "median and min over %d timed repetitions per variant, variants alternated in one process, milliseconds" % a.reps,
              "composed_and_loop_run_on": "a build of the parent commit (--parent-lib)" if a.parent_lib else "the product itself",
              "criterion": "median of new < min of the better of composed and loop",
              "host_threads": int(hip.lib.ckzg_hip_host_thread_budget()), "cpus_in_affinity_mask": len(os.sched_getaffinity(0)),
              "clocks_before": clocks(), "shapes": []}
    for G, per in (tuple(int(v) for v in sh.split("x")) for sh in a.shapes.split(",")):
        nb = G * per
        which = [(g + i) % 4 for g in range(G) for i in range(per)]
        blobs = b"".join(mat[w][0] for w in which)
        cms = b"".join(mat[w][1] for w in which)
        proofs = b"".join(mat[w][2] for w in which)
        cm_rows = np.frombuffer(cms, dtype=np.uint8).reshape(nb, 48)
        start = (C.c_uint64 * (G + 1))(*[per * g for g in range(G + 1)])
        cell_start = (C.c_uint64 * (G + 1))(*[128 * per * g for g in range(G + 1)])
        ok_g, st_g = (C.c_bool * G)(), (C.c_uint8 * G)()
        cells = C.create_string_buffer(nb * 128 * 2048)   # pageable, as a client's buffer would be
        st_b = (C.c_uint8 * nb)()
        blobs_at = C.create_string_buffer(blobs, len(blobs))       # (the same bytes, addressable by offset)
        proofs_at = C.create_string_buffer(proofs, len(proofs))

        def v_new(f=new_fn, api=hip):
            rc = f(ok_g, st_g, blobs, cms, proofs, start, C.c_uint64(G), api.sp)
            assert rc == 0 and all(ok_g), (rc, list(ok_g))

        def v_route(staged):
            os.environ[KNOB] = "1" if staged else "0"
            try:
                v_new(new_ab, ab)
            finally:
                del os.environ[KNOB]

        def v_composed():
            rc = cells_batch(cells, None, st_b, blobs, C.c_uint64(nb), old.sp)
            assert rc == 0, rc
            rep = np.repeat(cm_rows, 128, axis=0)                      # C'[128 i + k] = commitments[i]
            idx = np.tile(np.arange(128, dtype=np.uint64), nb)         # idx'[128 i + k] = k
            rc = cell_groups(ok_g, st_g, rep.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), cells, proofs,
                             cell_start, C.c_uint64(G), old.sp)
            assert rc == 0 and all(ok_g), (rc, list(ok_g))

        def v_loop():
            okb = C.c_bool(False)
            for g in range(G):
                for i in range(per):
                    b = g * per + i
                    rc = cells_one(C.byref(cells, i * 128 * 2048), None, C.byref(blobs_at, b * 131072), old.sp)
                    assert rc == 0, rc
                rep = np.repeat(cm_rows[g * per:(g + 1) * per], 128, axis=0)
                idx = np.tile(np.arange(128, dtype=np.uint64), per)
                rc = verify_one(C.byref(okb), rep.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), cells,
                                C.byref(proofs_at, g * per * 128 * 48), C.c_uint64(per * 128), old.sp)
                assert rc == 0 and okb.value, (g, rc)

        variants = [("new", v_new), ("composed", v_composed), ("loop", v_loop)]
        if ab and G == 1:
            variants += [("new_chunk", lambda: v_route(False)), ("new_staged", lambda: v_route(True))]
        for _, f in variants:   # warm-up: arenas, code objects, the worker pool
            f()
            f()
        times = {name: [] for name, _ in variants}
        for rep in range(a.reps):
            k = rep % len(variants)   # (every variant follows every other one in turn: no fixed predecessor)
            for name, f in variants[k:] + variants[:k]:
                t = time.perf_counter()
                f()
                times[name].append((time.perf_counter() - t) * 1e3)
        row = {"groups": G, "blobs_per_group": per}
        for name, _ in variants:
            row[name] = {"median_ms": round(statistics.median(times[name]), 3), "min_ms": round(min(times[name]), 3)}
        best = min(row["composed"]["min_ms"], row["loop"]["min_ms"])
        row["criterion_met"] = row["new"]["median_ms"] < best
        # one traced call: the stages of the new call
        with tempfile.TemporaryFile() as tmp:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            os.environ["CKZG_HIP_TRACE"] = "1"
            try:
                v_new()
            finally:
                del os.environ["CKZG_HIP_TRACE"]
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            marks = re.findall(r"\[ckzg-hip trace\] (verify_[a-z_]+): (.*) ([0-9.]+) ms", tmp.read().decode("utf-8", "replace"))
        stages = {}   # (a call of several chunks marks every stage once per chunk: summed)
        for what, name, ms in marks:
            key = "%s: %s" % (what, name)
            stages[key] = round(stages.get(key, 0.0) + float(ms), 3)
        row["traced_call_stages_ms"] = stages
        row["traced_call_chunks"] = max([sum(1 for w, n, _ in marks if (w, n) == (marks[0][0], marks[0][1]))] if marks else [0])
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    result["clocks_after"] = clocks()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    for api in {id(x): x for x in (hip, old, ab) if x}.values():
        api.close()


if __name__ == "__main__":
    main()
