"""ckzg_hip_verify_coset_kzg_proof_batch_locate (per-coset verdicts at batch cost, coset sizes 2^e, e = 0 .. 6) against the
road to a verdict per item that exists without it, at the C-ABI, same box, same process:

  e = 1 .. 5   a loop of single-item ckzg_hip_verify_coset_kzg_proof_batch calls (loops of more than 256 calls are
               extrapolated from a 256-call loop; the record says which)
  e = 0        ckzg_hip_verify_kzg_proof_batch_locate on the same items (z = the coset's one point)
  e = 6        ckzg_hip_verify_cell_kzg_proof_batch_locate

    python tools/bench_coset_locate.py [--out profiles/coset_locate_bench.json] [--parent-so PATH] [--runs 20]
    python tools/bench_coset_locate.py --sum-forms [--out ...]       (merges "sum_forms" into an existing record)

--parent-so: a build of the parent commit's library; the alternatives are then timed in that build (the new call exists
only in this one).  Without it they are timed in this build.
Per (e, items, false items in (0, 1, 8, all)): median and minimum wall time over --runs calls, the stats the call
reported and the launch form of the small sums (coset_locate_plan.hpp).  "faster" is claimed only where this call's
median is below the alternative's minimum.
--sum-forms: the l-term fixed-base sums alone (libcoset_locate_shim.so: cls_sum_forms, the product's k_msm_small<LPV> on a
prefix of a 64-point table), every (e, items, LPV in 4 / 8 / 16 / 64), kernel time between events, median of --runs
launches: the measurement behind the two rows of coset_locate_plan.hpp.  Prints JSON lines and writes --out."""
import argparse
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

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NAME = "ckzg_hip_verify_coset_kzg_proof_batch_locate"
BLOBS = 4


def timed(fn, runs):
    fn()   # warm-up (arena, code objects, the slot's table)
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3)}


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

    def case(self, e, n, nbad):
        """n items, coset i mod m of blob (i / m) mod BLOBS; nbad of them (or all) carry the proof of the next coset"""
        m, per = 8192 >> e, 32 << e
        proofs, evals = self.at(e)
        bad = set(range(n)) if nbad == "all" else set(random.Random(n).sample(range(n), nbad))
        cm, idx, ev, pf = [], [], [], []
        for i in range(n):
            b, c = (i // m) % BLOBS, i % m
            cm.append(self.commit[b])
            idx.append(c)
            ev.append(evals[b][per * c:per * (c + 1)])
            pf.append(proofs[b][(c + 1) % m if i in bad else c])
        return [i not in bad for i in range(n)], (b"".join(cm), (C.c_uint64 * n)(*idx), b"".join(ev), b"".join(pf))


def run_locate(hip, e, n, args, exp, runs):
    f = getattr(hip.lib, NAME)
    f.restype = C.c_int
    ok, st, stats = (C.c_bool * n)(), (C.c_uint8 * n)(), (C.c_uint64 * 3)()

    def call():
        assert f(ok, st, stats, *args, C.c_uint64(n), C.c_uint32(e), hip.sp) == 0
    row = timed(call, runs)
    assert list(ok) == exp
    row["stats"] = list(stats)
    return row


def alternative(old, e, n, args, runs):
    cm, idx, ev, pf = args
    if e == 0:
        from coset_expect import ext_domain_points
        zs = ext_domain_points()
        z = b"".join(zs[c].to_bytes(32, "big") for c in idx)
        f = old.lib.ckzg_hip_verify_kzg_proof_batch_locate
        f.restype = C.c_int
        ok, st, stats = (C.c_bool * n)(), (C.c_uint8 * n)(), (C.c_uint64 * 3)()
        row = timed(lambda: f(ok, st, stats, cm, z, ev, pf, C.c_uint64(n), old.sp), runs)
        assert all(ok)
        row["what"] = "ckzg_hip_verify_kzg_proof_batch_locate"
        return row
    if e == 6:
        f = old.lib.ckzg_hip_verify_cell_kzg_proof_batch_locate
        f.restype = C.c_int
        ok, st, stats = (C.c_bool * n)(), (C.c_uint8 * n)(), (C.c_uint64 * 3)()
        row = timed(lambda: f(ok, st, stats, cm, idx, ev, pf, C.c_uint64(n), old.sp), runs)
        assert all(ok)
        row["what"] = "ckzg_hip_verify_cell_kzg_proof_batch_locate"
        return row
    f = old.lib.ckzg_hip_verify_coset_kzg_proof_batch
    f.restype = C.c_int
    calls, per = min(n, 256), 32 << e
    one = [(cm[48 * i:48 * i + 48], (C.c_uint64 * 1)(idx[i]), ev[per * i:per * (i + 1)], pf[48 * i:48 * i + 48]) for i in range(calls)]
    ok = C.c_bool(False)

    def loop():
        for a in one:
            assert f(C.byref(ok), *a, C.c_uint64(1), C.c_uint32(e), old.sp) == 0 and ok.value
    row = timed(loop, runs)
    row["what"] = "loop of single-item ckzg_hip_verify_coset_kzg_proof_batch calls"
    row["calls_timed"] = calls
    if calls < n:
        row["extrapolated_from_calls"] = calls
        row["median_ms"] = round(row["median_ms"] * n / calls, 3)
        row["min_ms"] = round(row["min_ms"] * n / calls, 3)
    return row


def sum_forms(a):
    import g1_expect as gx
    import rlc_expect as rx
    lib = C.CDLL(os.path.join(ROOT, "c-kzg-4844_amd", "libcoset_locate_shim.so"))
    lib.cls_sum_forms.restype = C.c_int
    src = gx.G1Source(C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so")))
    rnd = random.Random(2)
    s = rnd.randrange(2, R)
    mono = b"".join(src.raw(pow(s, k, R)) for k in range(64))
    roots = rx.le32(rx.roots_of_unity())
    sizes = [int(x) for x in a.sum_sizes.split(",")]
    rows = []
    for e in range(7):
        l, m = 1 << e, 8192 >> e
        nmax = max(sizes)
        vals = rx.le32([rnd.randrange(R) for _ in range(nmax << e)])
        for n in sizes:
            idx = (C.c_uint32 * n)(*[i % m for i in range(n)])
            row = {"e": e, "items": n}
            for lpv in (4, 8, 16, 64):
                ms = (C.c_float * a.runs)()
                rc = lib.cls_sum_forms(ms, vals, idx, mono, roots, C.c_size_t(n), e, 10, lpv, a.runs)
                if rc != 0:
                    raise SystemExit("cls_sum_forms -> %d at e = %d, n = %d, lpv = %d: nothing more is launched" % (rc, e, n, lpv))
                row["lpv%d" % lpv] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}
            row["fastest"] = min((4, 8, 16, 64), key=lambda v: row["lpv%d" % v]["median_ms"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-so", default="")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", default="128,1024,8192")
    ap.add_argument("--es", default="0,1,2,3,4,5,6")
    ap.add_argument("--sum-forms", action="store_true")
    ap.add_argument("--sum-sizes", default="128,256,512,1024,2048,4096,8192")
    a = ap.parse_args()
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
    if a.sum_forms:
        res["sum_forms"] = {"what": "k_msm_small<LPV> alone, kernel time between events, 10-bit table, median and minimum of %d launches" % a.runs,
                            "rows": sum_forms(a)}
    else:
        mod = ge.load_package()
        hip = mod.Kzg(mod.HIP_SO)
        old = mod.Kzg(os.path.abspath(a.parent_so)) if a.parent_so else hip
        shim = C.CDLL(os.path.join(ROOT, "c-kzg-4844_amd", "csrc", "libhost_shim.so"))
        mat = Material(hip)
        res.update({"tool": "bench_coset_locate", "host_threads": int(hip.lib.ckzg_hip_host_thread_budget()),
                    "cpus_in_affinity_mask": len(os.sched_getaffinity(0)), "runs": a.runs,
                    "alternatives_timed_in": "parent build" if a.parent_so else "this build", "rows": []})
        for e in [int(x) for x in a.es.split(",")]:
            for n in [int(x) for x in a.sizes.split(",")]:
                exp, args = mat.case(e, n, 0)
                row = {"e": e, "items": n, "sum_lpv": shim.hs_coset_locate_sum_lpv(e, C.c_uint64(n)),
                       "alternative": alternative(old, e, n, args, a.runs), "locate": {}}
                for nbad in (0, 1, 8, "all"):
                    exp, args = mat.case(e, n, nbad)
                    row["locate"][str(nbad)] = run_locate(hip, e, n, args, exp, a.runs)
                row["faster_all_true"] = row["locate"]["0"]["median_ms"] < row["alternative"]["min_ms"]
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
        hip.close()
        if old is not hip:
            old.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
