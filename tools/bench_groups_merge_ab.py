"""The three grouped cell / coset verifications -- ckzg_hip_verify_cell_kzg_proof_batch_groups,
ckzg_hip_verify_blob_cell_kzg_proof_batch_groups and ckzg_hip_verify_coset_kzg_proof_batch_groups -- on two builds of the
library loaded in one process: this tree's and another (the parent commit's).  For a change that must leave all three
as fast as they were.

    python tools/bench_groups_merge_ab.py --alt PATH/libckzg_hip.so [--new OTHER.so] [--out FILE] [--reps 20] [--blocks 5]

Points (groups x units per group, valid data in pageable host memory, default tables): the cell entry at 128x8, 128x64,
8x64 and 512x1 cells; the blob-cell entry at 128x6, 8x6 and 64x1 blobs; the coset entry at e = 0, 3, 6 at 128x8 and 8x64
items.  Per point and block: two warm-up calls of each build, then `reps` timed calls of each, alternating alt, new,
alt, new ...; the median of the wall time (every call ends in a device synchronise).  The whole list runs `blocks`
times.  The margin of a point is the spread of the alternative's own block medians, maximum minus minimum; `within` says
whether the median of the new build's block medians exceeds that of the alternative's by no more than the margin.  The
verdicts of both builds are compared at every point.  Then one traced call of each build per point (CKZG_HIP_TRACE: the
call waits after every stage, so the marks are the stages' own times).  --new: another build in the place of this
tree's (a copy of the alternative: the control).  Prints one JSON object (and writes it to FILE)."""
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
BLOBS = 4
POINTS = ([("cell", 6, G, n) for G, n in ((128, 8), (128, 64), (8, 64), (512, 1))] +
          [("blob_cell", 6, G, n) for G, n in ((128, 6), (8, 6), (64, 1))] +
          [("coset", e, G, n) for e in (0, 3, 6) for G, n in ((128, 8), (8, 64))])
TRACE_NAME = {"cell": "verify_cell_groups", "blob_cell": "verify_blob_cell_groups", "coset": "verify_coset_groups"}


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


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
    out = {}   # (a call of several chunks marks every stage once per chunk: summed)
    for name, t in marks:
        out[name] = round(out.get(name, 0.0) + float(t), 3)
    return out


class Material:
    def __init__(self, k):
        rnd = random.Random(1)
        self.k = k
        self.blobs = [b"".join((rnd.randrange(R)).to_bytes(32, "big") for _ in range(4096)) for _ in range(BLOBS)]
        self.commit = [k.blob_to_kzg_commitment(b) for b in self.blobs]
        self.level = {}

    def at(self, e):
        if e not in self.level:
            proofs, evals, st = self.k.compute_coset_kzg_proofs_batch(self.blobs, e, want_evals=True)
            assert st == [0] * BLOBS
            self.level[e] = (proofs, evals)
        return self.level[e]

    def items(self, e, G, rows):
        """the PeerDAS shape: group g = coset g mod m of `rows` blobs (the base blobs repeated); flat arguments"""
        m, per = 8192 >> e, 32 << e
        proofs, evals = self.at(e)
        who = [(g % m, b % BLOBS) for g in range(G) for b in range(rows)]
        return (b"".join(self.commit[b] for _, b in who), (C.c_uint64 * len(who))(*[c for c, _ in who]),
                b"".join(evals[b][per * c:per * (c + 1)] for c, b in who), b"".join(proofs[b][c] for c, b in who))

    def blob_groups(self, G, per):
        """the shape of a transaction pool: a group is `per` blobs with their 128 cell proofs each"""
        proofs, _ = self.at(6)
        who = [(g + i) % BLOBS for g in range(G) for i in range(per)]
        return (b"".join(self.blobs[w] for w in who), b"".join(self.commit[w] for w in who),
                b"".join(b"".join(proofs[w]) for w in who))


def caller(k, kind, e, G, n, data):
    """(call, verdicts) of one point on the settings k"""
    start = (C.c_uint64 * (G + 1))(*[n * g for g in range(G + 1)])
    ok, st = (C.c_bool * G)(), (C.c_uint8 * G)()
    f = getattr(k.lib, {"cell": "ckzg_hip_verify_cell_kzg_proof_batch_groups",
                        "blob_cell": "ckzg_hip_verify_blob_cell_kzg_proof_batch_groups",
                        "coset": "ckzg_hip_verify_coset_kzg_proof_batch_groups"}[kind])
    f.restype = C.c_int
    tail = (start, C.c_uint64(G)) + ((C.c_uint32(e),) if kind == "coset" else ()) + (k.sp,)

    def call():
        rc = f(ok, st, *data, *tail)
        assert rc == 0 and all(ok), (kind, e, G, n, rc)

    return call, (ok, st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alt", required=True, help="the other build of libckzg_hip.so (the parent commit's)")
    ap.add_argument("--new", default="", help="a build in the place of this tree's (a copy of --alt: the control)")
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    mod = ge.load_package()
    new, alt = mod.Kzg(os.path.abspath(a.new) if a.new else mod.HIP_SO), mod.Kzg(os.path.abspath(a.alt))
    mat = Material(alt)
    res = {"tool": "bench_groups_merge_ab", "reps": a.reps, "blocks": a.blocks, "unit": "ms", "tables": "default",
           "alt": "the parent commit's build", "new": "a second copy of the parent commit's build" if a.new else "this tree's build",
           "order": "alt, new, alt, new, ... in one process", "host_threads": int(new.lib.ckzg_hip_host_thread_budget()),
           "cpus_in_affinity_mask": len(os.sched_getaffinity(0))}
    data = {p: mat.blob_groups(p[2], p[3]) if p[0] == "blob_cell" else mat.items(*p[1:]) for p in POINTS}
    med = {p: {"alt": [], "new": []} for p in POINTS}
    for _ in range(a.blocks):
        for p in POINTS:
            (ca, oa), (cn, on) = caller(alt, *p, data[p]), caller(new, *p, data[p])
            for _ in range(2):   # warm-up: arenas, code objects, the worker pool, the line table of [s^l]_2
                ca(), cn()
            assert [list(x) for x in oa] == [list(x) for x in on], "the two builds disagree at %s" % (p,)
            ta, tn = [], []
            for _ in range(a.reps):
                ta.append(ms(ca))
                tn.append(ms(cn))
            med[p]["alt"].append(round(statistics.median(ta), 3))
            med[p]["new"].append(round(statistics.median(tn), 3))
    rows = []
    for p in POINTS:
        kind, e, G, n = p
        ma, mn = med[p]["alt"], med[p]["new"]
        margin = round(max(ma) - min(ma), 3)
        over = round(statistics.median(mn) - statistics.median(ma), 3)
        row = {"call": kind, "log2_coset": e, "groups": G, "per_group": n, "alt_block_medians": ma, "new_block_medians": mn,
               "alt_median": statistics.median(ma), "new_median": statistics.median(mn), "margin": margin, "new_minus_alt": over,
               "within": over <= margin, "verdicts_equal": True}
        for name, k in (("alt", alt), ("new", new)):
            row[name + "_traced_call_stages_ms"] = traced(caller(k, *p, data[p])[0], TRACE_NAME[kind])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res["points"] = rows
    print(json.dumps({k: v for k, v in res.items() if k != "points"}))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    new.close()
    alt.close()


if __name__ == "__main__":
    main()
