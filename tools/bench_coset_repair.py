"""ckzg_hip_repair_cosets_and_kzg_proofs_rows (recovery by rows from untrusted cosets) at the C-ABI, default tables, a
fresh process.  Three modes.

Whole call (default):
    python tools/bench_coset_repair.py --parent-so PATH [--out profiles/coset_repair_bench.json] [--reps 20] [--es 0,3,6]
16 and 256 rows over 8 blobs, every row holding half of its cosets plus three (16 distinct sets), evaluations only and
with proofs.  Per configuration, in alternation, `reps` timed calls each (median and minimum of the wall time; the calls
return with the device idle) of
  parent_a, parent_b  ckzg_hip_recover_cosets_and_kzg_proofs_rows in --parent-so (a build of the parent commit loaded in
                      this process), two series: their difference is the run-to-run spread of the parent build;
  unchecked           the same entry in this build (must stay within that spread);
  checked             the new call, everything true, with commitments: `check_price` = checked - the mean of the parent's medians;
  repair_true         the new call, everything true, with commitments and the held cosets' proofs (no row fails, so no
                      pairing is spent);
  compose             what a client writes on the parent build: ckzg_hip_verify_coset_kzg_proof_batch_locate over all held
                      cosets, then the rows call;
and, evaluations only at 256 rows, the new call with one false coset in one row, one in every row, and every coset false
(`repair_one`, `repair_each`, `repair_all`).  A configuration whose warm-up takes more than --slow-ms runs --slow-reps
calls, one that takes more than --skip-ms is recorded from its warm-up alone.

One existing entry, once, for a kernel trace (--entry batch|cells_rows|cosets_rows, in --so or this build):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_coset_repair.py --entry cells_rows [--so PATH]
Compare two such traces by kernel name and count (adds "kernel_listing" to the JSON):
    python tools/bench_coset_repair.py --listing NAME=DIR_THIS,DIR_PARENT [NAME=...] [--out ...]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import random
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ROWS, REPAIR, LOCATE = ("ckzg_hip_recover_cosets_and_kzg_proofs_rows", "ckzg_hip_repair_cosets_and_kzg_proofs_rows",
                        "ckzg_hip_verify_coset_kzg_proof_batch_locate")


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(t):
    return round(statistics.median(t), 3), round(min(t), 3)


def blobs8():
    rnd = random.Random(3)
    return [b"".join((rnd.randrange(R)).to_bytes(32, "big") for _ in range(4096)) for _ in range(8)]


def run_calls(a):
    mod = ge.load_package()
    hip = mod.Kzg(mod.HIP_SO)
    old = mod.Kzg(os.path.abspath(a.parent_so))
    blobs = blobs8()
    cms = [hip.blob_to_kzg_commitment(b) for b in blobs]
    _, evals, st = hip.compute_coset_kzg_proofs_batch(blobs, 6, want_evals=True)
    assert st == [0] * 8
    res = {"tool": "bench_coset_repair", "reps": a.reps, "unit": "ms", "tables": "default", "blobs": 8,
           "held": "m / 2 + 3 cosets a row, 16 distinct sets", "parent_build": "loaded in the same process",
           "multi_device": "not measured"}
    rows_out = []
    rnd = random.Random(5)
    for e in [int(x) for x in a.es.split(",")]:
        m, item, l = 8192 >> e, 32 << e, 1 << e
        ext = [np.frombuffer(ev, dtype=np.uint8).reshape(m, item) for ev in evals]
        proofs, st = hip.compute_coset_kzg_proofs_batch(blobs, e)
        assert st == [0] * 8
        pr = [np.frombuffer(b"".join(p), dtype=np.uint8).reshape(m, 48) for p in proofs]
        per = m // 2 + 3
        for nrows in (16, 256):
            sets = [np.array(sorted(rnd.sample(range(m), per))) for _ in range(16)]
            idx = np.concatenate([sets[r % 16] for r in range(nrows)]).astype(np.uint64)
            data = b"".join(ext[r % 8][sets[r % 16]].tobytes() for r in range(nrows))
            held = b"".join(pr[r % 8][sets[r % 16]].tobytes() for r in range(nrows))
            row_cms = b"".join(cms[r % 8] for r in range(nrows))
            item_cms = b"".join(cms[r % 8] * per for r in range(nrows))
            start = (C.c_uint64 * (nrows + 1))(*[r * per for r in range(nrows + 1)])
            cidx = (C.c_uint64 * len(idx)).from_buffer_copy(idx.tobytes())
            n_items = nrows * per
            out_e, out_p = C.create_string_buffer(nrows * 8192 * 32), C.create_string_buffer(nrows * m * 48)
            status, verdict = (C.c_uint8 * nrows)(), (C.c_uint8 * nrows)()
            ok, lstat, rstat = (C.c_bool * n_items)(), (C.c_uint64 * 3)(), (C.c_uint64 * 4)()
            nr, ce = C.c_uint64(nrows), C.c_uint32(e)

            def unchecked(k, p, d=None):
                assert k._fn(ROWS)(out_e, p, status, cidx, d or data, start, nr, ce, k.sp) == 0

            def repair(p, d, hp, want=None):
                assert hip._fn(REPAIR)(out_e, p, status, verdict, ok if hp else None, rstat, cidx, d, start, nr, row_cms, hp, ce,
                                       hip.sp) == 0
                if want is not None:
                    assert sorted(set(verdict)) == want, sorted(set(verdict))

            def compose(p):
                assert old._fn(LOCATE)(ok, None, lstat, item_cms, cidx, data, held, C.c_uint64(n_items), ce, old.sp) == 0
                assert np.frombuffer(ok, dtype=np.uint8).all()
                unchecked(old, p)

            for want_proofs in (False, True):
                p = out_p if want_proofs else None
                series = {"parent_a": lambda: unchecked(old, p), "unchecked": lambda: unchecked(hip, p),
                          "checked": lambda: repair(p, data, None, [0]), "parent_b": lambda: unchecked(old, p),
                          "repair_true": lambda: repair(p, data, held, [0]), "compose": lambda: compose(p)}
                if not want_proofs and nrows == 256:
                    def flipped(cosets):   # the lowest bit of the first value of these held cosets
                        v = np.frombuffer(data, dtype=np.uint8).reshape(-1, 32).copy()
                        v[np.asarray(cosets) * l, 31] ^= 1
                        return v.tobytes()
                    one = flipped([7])
                    each = flipped([r * per + (r % per) for r in range(nrows)])
                    every = flipped(np.arange(n_items))
                    series["repair_one"] = lambda: repair(p, one, held, [0, 3])
                    series["repair_each"] = lambda: repair(p, each, held, [3])
                    series["repair_all"] = lambda: repair(p, every, held, [4])
                row = {"log2_coset": e, "rows": nrows, "proofs": want_proofs, "held_cosets": n_items}
                warm = {}
                for k, fn in series.items():
                    warm[k] = ms(fn)
                    if k in ("checked", "compose"):
                        assert out_e.raw[:8192 * 32] == evals[0]
                t = {k: [] for k in series}
                reps = {k: 0 if warm[k] > a.skip_ms else (a.slow_reps if warm[k] > a.slow_ms else a.reps) for k in series}
                for i in range(a.reps):
                    for k, fn in series.items():
                        if i < reps[k]:
                            t[k].append(ms(fn))
                for k in series:
                    med, mn = stats(t[k]) if t[k] else (round(warm[k], 3), round(warm[k], 3))
                    row[k] = {"median": med, "min": mn, "reps": reps[k] or "warm-up only"}
                pa, pb = row["parent_a"]["median"], row["parent_b"]["median"]
                row["parent_spread"] = round(abs(pa - pb), 3)
                row["unchecked_minus_parent"] = round(row["unchecked"]["median"] - (pa + pb) / 2, 3)
                row["unchecked_within_spread"] = min(pa, pb) - row["parent_spread"] <= row["unchecked"]["median"] <= max(pa, pb) + row["parent_spread"]
                row["check_price"] = round(row["checked"]["median"] - (pa + pb) / 2, 3)
                row["check_price_us_per_row"] = round(1e3 * row["check_price"] / nrows, 2)
                row["repair_true_faster_than_compose"] = row["repair_true"]["median"] < row["compose"]["min"]
                rows_out.append(row)
                print(json.dumps(row), flush=True)
                if a.out:   # after every row: a run that is cut short keeps what it has
                    keep = {}
                    if os.path.exists(a.out):
                        with open(a.out) as fh:
                            keep = {k: v for k, v in json.load(fh).items() if k == "kernel_listing"}
                    with open(a.out, "w") as fh:
                        json.dump(dict(res, rows=rows_out, **keep), fh, indent=1)
    old.close()
    hip.close()


def run_entry(a):
    """one call of one of the three existing recovery entries on 16 rows at e = 6, with proofs"""
    mod = ge.load_package()
    hip = mod.Kzg(os.path.abspath(a.so) if a.so else mod.HIP_SO)
    blobs = blobs8()
    _, evals, st = hip.compute_coset_kzg_proofs_batch(blobs, 6, want_evals=True)
    rnd = random.Random(11)
    nrows, per = 16, 67
    ext = [np.frombuffer(ev, dtype=np.uint8).reshape(128, 2048) for ev in evals]
    same = np.array(sorted(rnd.sample(range(128), per)))
    sets = [same] * 16 if a.entry == "batch" else [np.array(sorted(rnd.sample(range(128), per))) for _ in range(16)]
    idx = np.concatenate(sets).astype(np.uint64)
    data = b"".join(ext[r % 8][sets[r]].tobytes() for r in range(nrows))
    start = (C.c_uint64 * (nrows + 1))(*[r * per for r in range(nrows + 1)])
    cidx = (C.c_uint64 * len(idx)).from_buffer_copy(idx.tobytes())
    out_e, out_p, status = C.create_string_buffer(nrows * 8192 * 32), C.create_string_buffer(nrows * 128 * 48), (C.c_uint8 * nrows)()
    if a.entry == "batch":
        one = (C.c_uint64 * per)(*[int(c) for c in same])
        ret = hip._fn("ckzg_hip_recover_cells_and_kzg_proofs_batch")(out_e, out_p, status, one, data, C.c_uint64(per), C.c_uint64(nrows), hip.sp)
    elif a.entry == "cells_rows":
        ret = hip._fn("ckzg_hip_recover_cells_and_kzg_proofs_rows")(out_e, out_p, status, cidx, data, start, C.c_uint64(nrows), hip.sp)
    else:
        ret = hip._fn(ROWS)(out_e, out_p, status, cidx, data, start, C.c_uint64(nrows), C.c_uint32(6), hip.sp)
    assert ret == 0 and out_e.raw[:8192 * 32] == evals[0]
    hip.close()


def kernel_counts(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under " + d)
    counts = {}
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = re.sub(r"\s*\[clone.*$", "", r["Kernel_Name"])
                counts[name] = counts.get(name, 0) + 1
    return counts


def run_listing(a):
    out = {}
    for spec in a.listing:
        name, dirs = spec.split("=")
        this, parent = [kernel_counts(d) for d in dirs.split(",")]
        out[name] = {"same": this == parent, "launches": sum(this.values()), "kernels": dict(sorted(this.items()))}
        if this != parent:
            out[name]["parent_kernels"] = dict(sorted(parent.items()))
        print(name, "same" if this == parent else "DIFFERENT", sum(this.values()), "launches,", len(this), "kernels")
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    res["kernel_listing"] = {"from": "one rocprofv3 --kernel-trace run per entry and build: 16 rows at e = 6 with proofs, settings load included",
                             "entries": out}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coset_repair_bench.json"))
    ap.add_argument("--parent-so", default="")
    ap.add_argument("--so", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-ms", type=float, default=400.0)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--skip-ms", type=float, default=4000.0)
    ap.add_argument("--es", default="0,3,6")
    ap.add_argument("--entry", default="")
    ap.add_argument("--listing", nargs="*", default=[])
    a = ap.parse_args()
    if a.entry:
        run_entry(a)
    elif a.listing:
        run_listing(a)
    else:
        if not a.parent_so:
            raise SystemExit("--parent-so: the price of the check is measured against a build of the parent commit")
        run_calls(a)


if __name__ == "__main__":
    main()
