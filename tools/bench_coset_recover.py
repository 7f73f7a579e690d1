"""ckzg_hip_recover_cosets_and_kzg_proofs_rows (recovery by rows at any coset size 2^e) at the C-ABI, default tables, a
fresh process.  Two modes.

Whole call (default):
    python tools/bench_coset_recover.py [--out profiles/coset_recover_bench.json] [--parent-so PATH] [--reps 20] [--es 0,..,6]
16 and 256 rows over 8 blobs, every row holding half of its cosets plus three, with 1, 16 and 256 distinct sets (no more
than rows), evaluations only and with proofs, at every e.  Per row of the table one warm-up and `reps` timed calls,
median and minimum of the wall time (the call returns with the device idle).  A configuration whose warm-up takes more
than --slow-ms runs --slow-reps calls instead and says so.  At e = 6 the alternative,
ckzg_hip_recover_cells_and_kzg_proofs_rows over the same rows, alternates with further calls of the new one; it runs in
--parent-so (a build of the parent commit's library loaded in this process) if given, else in this build.  `faster` is
the README's standard: the new call's median below the alternative's minimum.

Factor kernel (--factors), for a run of its own under a kernel trace, with no counters:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_coset_recover.py --factors
    python tools/bench_coset_recover.py --trace DIR [--out ...]        (adds "factor_kernel" to the JSON of the first mode)
k_coset_recover_factors through libcoset_recover_shim.so (the product's object files) at e = 0, 3, 6 for 1, 16 and 256
sets of m / 2 missing cosets with the picker's `parts`, and every shape in which the picker splits (one set at each e,
2 and 4 sets at e = 0, 16 sets at e = 3 and 6, 256 sets at e = 6) next to the same launch with parts forced to 1: one
warm-up and `reps` launches each, in the order --factors prints, which is how --trace finds them in the trace.  The
shim takes `parts` as an argument, so the unsplit launch needs no second build and the product reads no tuning variable."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NAME = "ckzg_hip_recover_cosets_and_kzg_proofs_rows"
KERNEL = "k_coset_recover_factors"


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(t):
    return round(statistics.median(t), 3), round(min(t), 3)


def brp(v, bits):
    return int(format(v, "0%db" % bits)[::-1], 2)


def factor_configs():
    """(e, sets, parts forced or None for the picker's): the issue's grid, then every other shape in which the picker
    splits at 1 or 16 sets, each next to its unsplit launch"""
    out = [(e, sets, None) for e in (0, 3, 6) for sets in (1, 16, 256)]
    out += [(0, 1, 1), (0, 16, 1)]
    out += [(0, 2, None), (0, 2, 1), (0, 4, None), (0, 4, 1)]
    out += [(e, 1, None) for e in (1, 2, 4, 5)] + [(e, 1, 1) for e in range(1, 7)]
    return out + [(3, 16, 1), (6, 16, 1), (6, 256, 1)]


def picker(host, sets, e):
    host.hs_coset_recover_parts.restype = C.c_uint32
    return host.hs_coset_recover_parts(C.c_uint64(sets), C.c_int(e))


def run_factors(a):
    mod = ge.load_package()
    pkg = os.path.dirname(mod.HIP_SO)
    shim = C.CDLL(os.path.join(pkg, "libcoset_recover_shim.so"))
    host = C.CDLL(os.path.join(pkg, "csrc", "libhost_shim.so"))
    shim.crs_guard.restype = C.c_size_t
    G = shim.crs_guard()
    w = pow(7, (R - 1) // 8192, R)
    roots, v = [], 1
    for _ in range(8193):
        roots.append(v)
        v = v * w % R
    roots_raw = b"".join(x.to_bytes(32, "little") for x in roots)
    rnd = random.Random(9)
    for e, sets, forced in factor_configs():
        m = 8192 >> e
        parts = forced or picker(host, sets, e)
        miss, start = [], [0]
        for _ in range(sets):
            miss += [brp(j, 13 - e) << e for j in sorted(rnd.sample(range(m), m // 2))]
            start.append(len(miss))
        n = (sets * m + 2 * G) * 32
        zd, zi = C.create_string_buffer(n), C.create_string_buffer(n)
        seven_l = pow(7, 1 << e, R).to_bytes(32, "little")
        um, us = (C.c_uint32 * len(miss))(*miss), (C.c_uint32 * len(start))(*start)
        for _ in range(a.reps + 1):
            rc = C.c_int(-1)
            run = shim.crs_factors(zd, zi, um, us, C.c_size_t(sets), C.c_int(e), C.c_uint32(parts), roots_raw, seven_l, C.byref(rc))
            if run != 0 or rc.value != 0:
                raise SystemExit("crs_factors returned %d / %d" % (run, rc.value))
        print(json.dumps({"log2_coset": e, "sets": sets, "parts": parts, "forced": forced is not None, "launches": a.reps + 1}),
              flush=True)


def read_trace(a):
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under " + a.trace)
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if KERNEL in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    rows.sort()
    host = C.CDLL(os.path.join(os.path.dirname(ge.load_package().HIP_SO), "csrc", "libhost_shim.so"))
    per = a.reps + 1
    cfgs = factor_configs()
    if len(rows) != per * len(cfgs):
        raise SystemExit("%d launches of %s in the trace, expected %d" % (len(rows), KERNEL, per * len(cfgs)))
    out = []
    for i, (e, sets, forced) in enumerate(cfgs):
        t = [d for _, d in rows[i * per + 1:(i + 1) * per]]      # without the warm-up
        med, mn = stats(t)
        out.append({"log2_coset": e, "sets": sets, "parts": forced or picker(host, sets, e),
                    "parts_forced_to_1": forced is not None, "kernel_median_ms": med,
                    "kernel_min_ms": mn, "ms_per_set": round(med / sets, 4)})
        print(json.dumps(out[-1]), flush=True)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    res["factor_kernel"] = {"from": "one rocprofv3 --kernel-trace --stats run, no counters", "reps": a.reps, "rows": out}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


def run_calls(a):
    mod = ge.load_package()
    hip = mod.Kzg(mod.HIP_SO)
    old = mod.Kzg(os.path.abspath(a.parent_so)) if a.parent_so else hip
    rnd = random.Random(3)
    blobs = [b"".join((rnd.randrange(R)).to_bytes(32, "big") for _ in range(4096)) for _ in range(8)]
    _, evals, st = hip.compute_coset_kzg_proofs_batch(blobs, 6, want_evals=True)
    assert st == [0] * 8
    f, g = hip._fn(NAME), old._fn("ckzg_hip_recover_cells_and_kzg_proofs_rows")
    res = {"tool": "bench_coset_recover", "reps": a.reps, "unit": "ms", "tables": "default", "blobs": 8,
           "held": "m / 2 + 3 cosets a row", "alternative_timed_in": "parent build" if a.parent_so else "this build"}
    rows_out = []
    for e in [int(x) for x in a.es.split(",")]:
        m, item = 8192 >> e, 32 << e
        ext = [np.frombuffer(ev, dtype=np.uint8).reshape(m, item) for ev in evals]
        for nrows, nsets in ((16, 1), (16, 16), (256, 1), (256, 16), (256, 256)):
            sets = [np.array(sorted(rnd.sample(range(m), m // 2 + 3))) for _ in range(nsets)]
            idx = np.concatenate([sets[r % nsets] for r in range(nrows)]).astype(np.uint64)
            data = b"".join(ext[r % 8][sets[r % nsets]].tobytes() for r in range(nrows))
            start = (C.c_uint64 * (nrows + 1))(*[r * (m // 2 + 3) for r in range(nrows + 1)])
            cidx = (C.c_uint64 * len(idx)).from_buffer_copy(idx.tobytes())
            out_e, out_p = C.create_string_buffer(nrows * 8192 * 32), C.create_string_buffer(nrows * m * 48)
            status = (C.c_uint8 * nrows)()
            for want_proofs in (False, True):
                def new():
                    assert f(out_e, out_p if want_proofs else None, status, cidx, data, start, C.c_uint64(nrows),
                             C.c_uint32(e), hip.sp) == 0
                warm = ms(new)
                assert out_e.raw[:8192 * 32] == evals[0]
                reps = a.reps if warm <= a.slow_ms else a.slow_reps
                tn = [ms(new) for _ in range(reps)]
                row = {"log2_coset": e, "rows": nrows, "distinct_sets": nsets, "proofs": want_proofs, "reps": reps}
                if e == 6:
                    alt_p = C.create_string_buffer(nrows * 128 * 48)

                    def alt():
                        assert g(out_e, alt_p if want_proofs else None, status, cidx, data, start, C.c_uint64(nrows), old.sp) == 0
                    alt()
                    if want_proofs:
                        assert alt_p.raw == out_p.raw
                    to = []
                    for _ in range(reps):   # alternating with the new call, whose time is taken again next to it
                        to.append(ms(alt))
                        tn.append(ms(new))
                    row["alt"] = "ckzg_hip_recover_cells_and_kzg_proofs_rows"
                    row["alt_median"], row["alt_min"] = stats(to)
                row["new_median"], row["new_min"] = stats(tn)
                row["new_ms_per_row"] = round(row["new_median"] / nrows, 4)
                if e == 6:
                    row["faster"] = row["new_median"] < row["alt_min"]
                    row["new_median_over_alt_min"] = round(row["new_median"] / row["alt_min"], 3)
                rows_out.append(row)
                print(json.dumps(row), flush=True)
    res["rows"] = rows_out
    if a.out:
        keep = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                keep = {k: v for k, v in json.load(fh).items() if k == "factor_kernel"}
        res.update(keep)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if old is not hip:
        old.close()
    hip.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coset_recover_bench.json"))
    ap.add_argument("--parent-so", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-ms", type=float, default=400.0)
    ap.add_argument("--slow-reps", type=int, default=5)
    ap.add_argument("--es", default="0,1,2,3,4,5,6")
    ap.add_argument("--factors", action="store_true")
    ap.add_argument("--trace", default="")
    a = ap.parse_args()
    if a.factors:
        run_factors(a)
    elif a.trace:
        read_trace(a)
    else:
        run_calls(a)


if __name__ == "__main__":
    main()
