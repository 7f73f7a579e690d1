"""ckzg_hip_recover_cells_and_kzg_proofs_rows (rows that hold different cells in one call) against what a caller had
before it, at the C-ABI, pageable host buffers in and out, with the table widths of tools/bench_recover.py
(fk20_wbits 12, proof_wbits 13: the setting of the README's recovery row).

    python tools/bench_recover_rows.py [--out FILE] [--reps 20] [--rows 256] [--sets 1,8,64,256]
    python tools/bench_recover_rows.py --trace            (the workload of a rocprofv3 --kernel-trace --stats run)
    python tools/bench_recover_rows.py --merge-stats kernel_stats.csv --out FILE

Per S (distinct sets of 64..96 cells, row r on set r mod S) the variants are alternated in one process, `--reps`
timed repetitions of each after a warm-up round; median and min in milliseconds:
    rows       the new call, rows in their given (interleaved) order
    per_set    the way of the parent commit: rows sorted by set beforehand (not timed), one
               ckzg_hip_recover_cells_and_kzg_proofs_batch call per set -- the yardstick
    one_row    one recover_cells_and_kzg_proofs call per row
and at S = 1 also
    batch, batch_again   ckzg_hip_recover_cells_and_kzg_proofs_batch itself, twice in the rotation: the difference of
               the two medians is the run-to-run spread that `rows` is allowed against `batch`.
Every variant's output is compared with the full rows before timing.  --trace runs a warm-up, then one `rows` call at
S = 256 and one one-row batch call (whose k_fr_div_inplace and two single-vector transforms are what the set-factor
kernel replaces per set); --merge-stats copies the recovery kernels' lines of that run's kernel_stats.csv into FILE."""
import argparse
import csv
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

CELLS, PROOFS = 128 * 2048, 128 * 48
KERNELS = ("k_coset_recover_factors", "k_scatter_cosets_rows", "k_fr_mul_coset_factor", "k_fr_mul_inplace", "k_fr_div_inplace",
           "k_scatter_cells", "k_ntt_tile", "k_ntt8192_outer", "k_bytes_to_fr", "k_fr_to_bytes")


class Work:
    def __init__(self, api, full, nr, nsets, seed=1):
        rnd = random.Random(seed * 1000 + nsets)
        sets = set()
        while len(sets) < nsets:
            sets.add(tuple(sorted(rnd.sample(range(128), rnd.randrange(64, 97)))))
        self.sets = sorted(sets, key=lambda s: rnd.random())
        self.api, self.nr, self.full = api, nr, full
        self.row_set = [r % nsets for r in range(nr)]
        self.row_blob = [r % len(full) for r in range(nr)]
        cut = {}

        def cells_of(r):
            key = (self.row_blob[r], self.row_set[r])
            if key not in cut:
                cut[key] = b"".join(full[key[0]][0][c] for c in self.sets[key[1]])
            return cut[key]

        # the new call: rows as they come
        idx = [c for r in range(nr) for c in self.sets[self.row_set[r]]]
        start = [0]
        for r in range(nr):
            start.append(start[-1] + len(self.sets[self.row_set[r]]))
        self.idx = (C.c_uint64 * len(idx))(*idx)
        self.start = (C.c_uint64 * (nr + 1))(*start)
        self.data = b"".join(cells_of(r) for r in range(nr))
        # the parent's way: rows sorted by set, one contiguous input and output region per set
        self.by_set = []
        off = 0
        for s in range(nsets):
            members = [r for r in range(nr) if self.row_set[r] == s]
            self.by_set.append(((C.c_uint64 * len(self.sets[s]))(*self.sets[s]), len(self.sets[s]),
                                b"".join(cells_of(r) for r in members), members, off))
            off += len(members)
        self.one = [((C.c_uint64 * len(self.sets[self.row_set[r]]))(*self.sets[self.row_set[r]]),
                     len(self.sets[self.row_set[r]]), cells_of(r)) for r in range(nr)]
        self.rc = C.create_string_buffer(nr * CELLS)
        self.rp = C.create_string_buffer(nr * PROOFS)
        lib = api.lib
        self.f_rows = lib.ckzg_hip_recover_cells_and_kzg_proofs_rows
        self.f_batch = lib.ckzg_hip_recover_cells_and_kzg_proofs_batch
        self.f_one = lib.recover_cells_and_kzg_proofs
        for f in (self.f_rows, self.f_batch, self.f_one):
            f.restype = C.c_int

    def rows(self):
        assert self.f_rows(self.rc, self.rp, None, self.idx, self.data, self.start, C.c_uint64(self.nr), self.api.sp) == 0
        return list(range(self.nr))

    def per_set(self):
        order = []
        for idx, n, data, members, off in self.by_set:
            rc = (C.c_char * (len(members) * CELLS)).from_buffer(self.rc, off * CELLS)
            rp = (C.c_char * (len(members) * PROOFS)).from_buffer(self.rp, off * PROOFS)
            assert self.f_batch(rc, rp, None, idx, data, C.c_uint64(n), C.c_uint64(len(members)), self.api.sp) == 0
            order.extend(members)
        return order

    batch = batch_again = per_set   # (at S = 1 the loop is one call of the existing entry point)

    def one_row(self):
        for r, (idx, n, data) in enumerate(self.one):
            rc = (C.c_char * CELLS).from_buffer(self.rc, r * CELLS)
            rp = (C.c_char * PROOFS).from_buffer(self.rp, r * PROOFS)
            assert self.f_one(rc, rp, idx, data, C.c_uint64(n), self.api.sp) == 0
        return list(range(self.nr))

    def check(self, order):
        craw, praw = self.rc.raw, self.rp.raw
        want = [(b"".join(c), b"".join(p)) for c, p in self.full]
        for pos, r in enumerate(order):
            wc, wp = want[self.row_blob[r]]
            assert craw[pos * CELLS:(pos + 1) * CELLS] == wc and praw[pos * PROOFS:(pos + 1) * PROOFS] == wp, (pos, r)


def material(api, n=8):
    from test_gpu_commitment import rand_blob
    return [api.compute_cells_and_kzg_proofs(rand_blob(70, i)) for i in range(n)]


def merge_stats(path, out):
    rep = json.load(open(out)) if os.path.exists(out) else {}
    rows = {}
    for line in csv.DictReader(open(path)):
        if any(k in line["Name"] for k in KERNELS):
            short = line["Name"].split("(")[0].split("::")[-1]
            rows[short] = {"calls": int(line["Calls"]), "total_us": round(int(line["TotalDurationNs"]) / 1e3, 1),
                           "average_us": round(float(line["AverageNs"]) / 1e3, 2), "min_us": round(int(line["MinNs"]) / 1e3, 2),
                           "max_us": round(int(line["MaxNs"]) / 1e3, 2)}
    rep["kernel_trace"] = {
        "what": "rocprofv3 --kernel-trace --stats over tools/bench_recover_rows.py --trace: compute_cells_and_kzg_proofs of "
                "8 blobs, then 2 rows calls (256 rows, 256 sets; the first a warm-up) and 2 one-row batch calls",
        "kernels": rows}
    json.dump(rep, open(out, "w"), indent=1)
    print(json.dumps(rep["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--sets", default="1,8,64,256")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--merge-stats", default="")
    a = ap.parse_args()
    if a.merge_stats:
        return merge_stats(a.merge_stats, a.out)
    mod = ge.load_package()
    api = mod.Kzg(options={"fk20_wbits": 12, "proof_wbits": 13})
    full = material(api)
    if a.trace:
        w = Work(api, full, a.rows, min(256, a.rows))
        for _ in range(2):
            w.check(w.rows())
        one = Work(api, full, 1, 1)
        for _ in range(2):
            one.check(one.per_set())
        api.close()
        print(json.dumps({"traced": "2 x rows(%d rows, %d sets), 2 x batch(1 row)" % (a.rows, len(w.sets))}))
        return
    rep = {"tool": "tools/bench_recover_rows.py --reps %d --rows %d --sets %s" % (a.reps, a.rows, a.sets),
           "box": "one MI355X; pageable host buffers in and out; fk20_wbits 12, proof_wbits 13",
           "stat": "median and min over %d timed repetitions per variant after one warm-up round, variants alternated, "
                   "milliseconds; cells and proofs both asked for" % a.reps,
           "variants": {"rows": "ckzg_hip_recover_cells_and_kzg_proofs_rows, one call, rows interleaved over the sets",
                        "per_set": "rows sorted by set (not timed), one ckzg_hip_recover_cells_and_kzg_proofs_batch per set",
                        "one_row": "one recover_cells_and_kzg_proofs per row",
                        "batch / batch_again": "S = 1: the existing batch call, twice in the rotation (run-to-run spread)"},
           "shapes": []}
    for nsets in [int(v) for v in a.sets.split(",")]:
        w = Work(api, full, a.rows, nsets)
        names = ["rows", "batch", "one_row", "batch_again"] if nsets == 1 else ["rows", "per_set", "one_row"]
        for name in names:   # warm-up round, checked
            w.check(getattr(w, name)())
        times = {name: [] for name in names}
        for _ in range(a.reps):
            for name in names:
                t = time.perf_counter()
                getattr(w, name)()
                times[name].append((time.perf_counter() - t) * 1e3)
        shape = {"rows": a.rows, "sets": nsets, "cells_per_row_mean": round(sum(len(s) for s in w.sets) / len(w.sets), 1)}
        for name in names:
            med = statistics.median(times[name])
            shape[name] = {"median_ms": round(med, 3), "min_ms": round(min(times[name]), 3), "rows_per_s": round(a.rows / med * 1e3)}
        yard = "batch" if nsets == 1 else "per_set"
        shape["yardstick"] = yard
        shape["yardstick_over_rows_median"] = round(shape[yard]["median_ms"] / shape["rows"]["median_ms"], 3)
        shape["one_row_over_rows_median"] = round(shape["one_row"]["median_ms"] / shape["rows"]["median_ms"], 3)
        if nsets == 1:
            shape["spread_of_batch_medians_ms"] = round(abs(shape["batch"]["median_ms"] - shape["batch_again"]["median_ms"]), 3)
            shape["rows_minus_batch_median_ms"] = round(shape["rows"]["median_ms"] - shape["batch"]["median_ms"], 3)
        rep["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
    api.close()
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        if "kernel_trace" in old:
            rep["kernel_trace"] = old["kernel_trace"]
        json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
