"""ckzg_hip_verify_coset_kzg_proof_batch (a batch of coset multiproofs checked at any coset size 2^e) at the C-ABI:
every e = 0 .. 6 at 128 / 1,024 / 8,192 items, all true and with one false item, default tables, a fresh process.  At
the two ends what a client had before it, in the same process on the same settings:

    e = 6   verify_cell_kzg_proof_batch over the same items (true and one false): the same pipeline, so the two tie
    e = 0   ckzg_hip_verify_kzg_proof_batch_locate with everything true: the cheapest public route to "are all of these
            right" for single points
    e = 1 .. 5   nothing: the library had no verifier for these sizes

    python tools/bench_coset_verify.py [--out profiles/coset_verify_bench.json] [--sizes 128,1024,8192] [--reps 20]

Per (e, size, kind): one warm-up and `reps` timed calls, median and minimum of the wall time (the call returns its
verdict, so every call ends with the device idle).  Where an alternative runs it alternates with further calls of the
new one.  `faster` is the README's standard: the new call's median below the alternative's minimum.  The items are the
openings of two blobs from ckzg_hip_compute_coset_kzg_proofs_batch, both commitments interleaved, every coset of a blob
before the next copy.  Prints one JSON object per row and the whole result (and writes it to --out)."""
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
import __graft_entry__ as ge  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def fr(v):
    return (v % R).to_bytes(32, "big")


def brp(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(t):
    return round(statistics.median(t), 3), round(min(t), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coset_verify_bench.json"))
    ap.add_argument("--sizes", default="128,1024,8192")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    mod = ge.load_package()
    rnd = random.Random(2)
    blobs = [b"".join(fr(rnd.randrange(R)) for _ in range(4096)) for _ in range(2)]
    w = pow(7, (R - 1) // 8192, R)
    pw = [1] * 8192
    for i in range(1, 8192):
        pw[i] = pw[i - 1] * w % R
    ext = [fr(pw[brp(j, 13)]) for j in range(8192)]
    sizes = [int(x) for x in a.sizes.split(",")]
    hip = mod.Kzg(mod.HIP_SO)
    commit = [hip.blob_to_kzg_commitment(b) for b in blobs]
    f = hip._fn("ckzg_hip_verify_coset_kzg_proof_batch")
    g_cell = hip._fn("verify_cell_kzg_proof_batch")
    g_locate = hip._fn("ckzg_hip_verify_kzg_proof_batch_locate")
    res = {"tool": "bench_coset_verify", "reps": a.reps, "unit": "ms", "tables": "default",
           "sums": "ladders; at e = 6 table sums from 128 items on (the pipeline of verify_cell_kzg_proof_batch)"}
    rows = []
    for e in range(7):
        l, m = 1 << e, 8192 >> e
        proofs, evals, st = hip.compute_coset_kzg_proofs_batch(blobs, e, want_evals=True)
        assert st == [0, 0]
        for n in sizes:
            who = [((i // m) % 2, i % m) for i in range(n)]
            cm = b"".join(commit[b] for b, _ in who)
            idx = (C.c_uint64 * n)(*[c for _, c in who])
            pf = b"".join(proofs[b][c] for b, c in who)
            ev_true = b"".join(evals[b][32 * l * c:32 * l * (c + 1)] for b, c in who)
            at = 32 * l * (n // 2) + 32 * (l - 1)
            ev_false = ev_true[:at] + fr(int.from_bytes(ev_true[at:at + 32], "big") + 1) + ev_true[at + 32:]
            for kind, ev, want in (("all true", ev_true, True), ("one false", ev_false, False)):
                ok = C.c_bool(False)

                def new():
                    assert f(C.byref(ok), cm, idx, ev, pf, C.c_uint64(n), C.c_uint32(e), hip.sp) == 0 and ok.value is want
                new()
                tn = [ms(new) for _ in range(a.reps)]
                row = {"log2_coset": e, "items": n, "kind": kind}
                old = None
                if e == 6:
                    def old():
                        assert g_cell(C.byref(ok), cm, idx, ev, pf, C.c_uint64(n), hip.sp) == 0 and ok.value is want
                    row["alt"] = "verify_cell_kzg_proof_batch"
                elif e == 0 and want:
                    zs = b"".join(ext[c] for _, c in who)
                    oks, sts, stat3 = (C.c_bool * n)(), (C.c_uint8 * n)(), (C.c_uint64 * 3)()

                    def old():
                        assert g_locate(oks, sts, stat3, cm, zs, ev, pf, C.c_uint64(n), hip.sp) == 0 and all(oks)
                    row["alt"] = "ckzg_hip_verify_kzg_proof_batch_locate"
                if old:
                    old()
                    to = []
                    for _ in range(a.reps):   # alternating with the new call, whose time is taken again next to it
                        to.append(ms(old))
                        tn.append(ms(new))
                    row["alt_median"], row["alt_min"] = stats(to)
                row["new_median"], row["new_min"] = stats(tn)
                row["new_us_per_item"] = round(1e3 * row["new_median"] / n, 3)
                if old:
                    row["faster"] = row["new_median"] < row["alt_min"]
                    row["alt_min_over_new_median"] = round(row["alt_min"] / row["new_median"], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
    res["rows"] = rows
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    hip.close()


if __name__ == "__main__":
    main()
