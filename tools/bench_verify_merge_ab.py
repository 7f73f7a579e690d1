"""A set of calls on two builds of the library, this tree's and another (the parent commit's), each in fresh processes
that take turns.  For a change that must leave the cell call as fast as it was.

    python tools/bench_verify_merge_ab.py --alt PATH/libckzg_hip.so [--points verify|recover] [--out FILE] [--reps 20] [--rounds 3]

Points of `verify` (verify_cell_kzg_proof_batch and ckzg_hip_verify_coset_kzg_proof_batch, default tables): the cell
call at 1, 16, 64, 127, 128, 1024, 4096 and 8192 cells (all true, 8 blobs' cells repeated); the coset
call at e = 0, 3, 6 at 128, 1024 and 8192 items (all true, the openings of two blobs interleaved).
Points of `recover` (recovery by rows; the workload and table widths of tools/bench_recover_rows.py, every output
compared with the full rows in the warm-up call): ckzg_hip_recover_cells_and_kzg_proofs_rows at 16 and 256 rows on 1,
16 and 256 distinct sets (16 rows hold at most 16), cells only and cells + proofs, at 1030 rows on 5 sets and at 512
rows on 512 sets, cells only; ckzg_hip_recover_cosets_and_kzg_proofs_rows at e = 6 at 16 and 256 rows on 16 sets with
proofs, and at e = 0 and e = 3 at 256 rows on 16 sets, evaluations only.  A round is one
fresh process of the alternative, then one of this tree's build; a process loads the library with default tables and,
per point, makes one warm-up call and `reps` timed ones and reports the median of the wall time (the call returns its
verdict, so every call ends with the device idle).  `rounds` rounds.  The margin of a point is the spread of the
alternative's own medians over its processes, maximum minus minimum; `within` says whether the median of this tree's
medians exceeds the median of the alternative's by no more than that margin.  Prints one JSON object (and writes it
to FILE); --bench adds one figure of one `bench.py --full` run of each build: verify_cell_kzg_proof_batch_n8192, or
for `recover` recover_cells_and_kzg_proofs_batch256 (the same-cells batch, which no by-rows change may move)."""
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

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
CELL_SIZES = [1, 16, 64, 127, 128, 1024, 4096, 8192]
COSET_ES = [0, 3, 6]
COSET_SIZES = [128, 1024, 8192]


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def timed(call, reps):
    call()
    return round(statistics.median(ms(call) for _ in range(reps)), 4)


def recover_points(so, reps):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_recover_rows as br
    hip = br.ge.load_package().Kzg(so, options={"fk20_wbits": 12, "proof_wbits": 13})
    full = br.material(hip)
    out = {}
    for nr, nsets, proofs in ([(nr, ns, pf) for nr in (16, 256) for ns in (1, 16, 256) if ns <= max(nr, 16) for pf in (False, True)]
                              + [(1030, 5, False), (512, 512, False)]):
        w = br.Work(hip, full, nr, nsets)
        rp = w.rp if proofs else None

        def call():
            assert w.f_rows(w.rc, rp, None, w.idx, w.data, w.start, C.c_uint64(nr), hip.sp) == 0
        call()
        want = [(b"".join(c), b"".join(p)) for c, p in full]
        for r in range(nr):
            assert w.rc[r * br.CELLS:(r + 1) * br.CELLS] == want[r % len(full)][0], r
            assert not proofs or w.rp[r * br.PROOFS:(r + 1) * br.PROOFS] == want[r % len(full)][1], r
        out["cells rows=%d sets=%d %s" % (nr, nsets, "cells+proofs" if proofs else "cells only")] = timed(call, reps)
    f = hip._fn("ckzg_hip_recover_cosets_and_kzg_proofs_rows")
    ext = [b"".join(c) for c, _ in full]
    for e, nr, proofs in [(6, 16, True), (6, 256, True), (0, 256, False), (3, 256, False)]:
        m, item, nsets = 8192 >> e, 32 << e, 16
        rnd = random.Random(100 + e)
        sets = [sorted(rnd.sample(range(m), rnd.randrange(m // 2, 3 * m // 4 + 1))) for _ in range(nsets)]
        cut = {}
        for r in range(nr):
            key = (r % len(full), r % nsets)
            if key not in cut:
                cut[key] = b"".join(ext[key[0]][c * item:(c + 1) * item] for c in sets[key[1]])
        data = b"".join(cut[(r % len(full), r % nsets)] for r in range(nr))
        flat = [c for r in range(nr) for c in sets[r % nsets]]
        start = [0]
        for r in range(nr):
            start.append(start[-1] + len(sets[r % nsets]))
        idx, st = (C.c_uint64 * len(flat))(*flat), (C.c_uint64 * (nr + 1))(*start)
        rv = C.create_string_buffer(nr * 8192 * 32)
        rp = C.create_string_buffer(nr * m * 48) if proofs else None

        def call():
            assert f(rv, rp, None, idx, data, st, C.c_uint64(nr), C.c_uint32(e), hip.sp) == 0
        call()
        for r in range(nr):
            assert rv[r * 262144:(r + 1) * 262144] == ext[r % len(full)], r
            assert not proofs or rp[r * br.PROOFS:(r + 1) * br.PROOFS] == b"".join(full[r % len(full)][1]), r
        out["cosets e=%d rows=%d sets=%d %s" % (e, nr, nsets, "evals+proofs" if proofs else "evals only")] = timed(call, reps)
    hip.close()
    print("AB " + json.dumps(out), flush=True)


def child(so, reps, points):
    """the medians of every point on the build `so`, as one JSON line"""
    if points == "recover":
        return recover_points(so, reps)
    import __graft_entry__ as ge
    mod = ge.load_package()
    hip = mod.Kzg(so)
    rnd = random.Random(3)
    blobs = [b"".join(rnd.randrange(R).to_bytes(32, "big") for _ in range(4096)) for _ in range(8)]
    commit = [hip.blob_to_kzg_commitment(b) for b in blobs]
    out = {}
    ok = C.c_bool(False)

    cp = [hip.compute_cells_and_kzg_proofs(b) for b in blobs]
    g = hip._fn("verify_cell_kzg_proof_batch")
    for n in CELL_SIZES:
        who = [((i // 128) % 8, i % 128) for i in range(n)]
        cm = b"".join(commit[b] for b, _ in who)
        idx = (C.c_uint64 * n)(*[c for _, c in who])
        cells = b"".join(cp[b][0][c] for b, c in who)
        pf = b"".join(cp[b][1][c] for b, c in who)

        def call():
            assert g(C.byref(ok), cm, idx, cells, pf, C.c_uint64(n), hip.sp) == 0 and ok.value is True
        out["cells n=%d" % n] = timed(call, reps)
    f = hip._fn("ckzg_hip_verify_coset_kzg_proof_batch")
    for e in COSET_ES:
        l, m = 1 << e, 8192 >> e
        proofs, evals, st = hip.compute_coset_kzg_proofs_batch(blobs[:2], e, want_evals=True)
        assert st == [0, 0]
        for n in COSET_SIZES:
            who = [((i // m) % 2, i % m) for i in range(n)]
            cm = b"".join(commit[b] for b, _ in who)
            idx = (C.c_uint64 * n)(*[c for _, c in who])
            pf = b"".join(proofs[b][c] for b, c in who)
            ev = b"".join(evals[b][32 * l * c:32 * l * (c + 1)] for b, c in who)

            def call():
                assert f(C.byref(ok), cm, idx, ev, pf, C.c_uint64(n), C.c_uint32(e), hip.sp) == 0 and ok.value is True
            out["cosets e=%d n=%d" % (e, n)] = timed(call, reps)
    hip.close()
    print("AB " + json.dumps(out), flush=True)


def run_child(so, reps, points):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", so, "--reps", str(reps), "--points", points],
                       capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("AB ")]
    if p.returncode != 0 or not lines:
        raise SystemExit("a measuring process on %s ended with %d:\n%s" % (so, p.returncode, p.stderr[-2000:]))
    return json.loads(lines[-1][3:])


def bench_figure(so, points):
    """one bench.py --full run (its secondary rows) on the build `so`: verify_cell_kzg_proof_batch_n8192, or the recover rows"""
    env = dict(os.environ, CKZG_HIP_SO=so)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--no-pcie"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    for ln in reversed(p.stdout.splitlines()):
        if ln.startswith("{"):
            line = json.loads(ln)
            sec = line.get("secondary")
            if not isinstance(sec, dict) and line.get("secondary_file"):
                sec = json.load(open(os.path.join(ROOT, line["secondary_file"]))).get("secondary")
            if points == "recover":
                return (sec or {}).get("recover_cells_and_kzg_proofs_batch256")
            return (sec or {}).get("verify_cell_kzg_proof_batch_n8192")
    raise SystemExit("bench.py on %s ended with %d:\n%s" % (so, p.returncode, p.stderr[-2000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alt", help="the other build of libckzg_hip.so (the parent commit's)")
    ap.add_argument("--child", help="(internal) measure this build and print its medians")
    ap.add_argument("--points", choices=["verify", "recover"], default="verify")
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", action="store_true", help="also one bench.py --full run of each build")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.points)
    if not a.alt:
        ap.error("--alt is required")
    import __graft_entry__ as ge
    new_so, alt_so = ge.load_package().HIP_SO, os.path.abspath(a.alt)
    res = {"tool": "bench_verify_merge_ab --points " + a.points, "reps": a.reps, "rounds": a.rounds, "unit": "ms",
           "tables": "default" if a.points == "verify" else "fk20_wbits 12, proof_wbits 13",
           "alt": "the parent commit's build", "new": "this tree's build", "order": "alt, new, alt, new, ... one fresh process each"}
    alt, new = [], []
    for i in range(a.rounds):
        alt.append(run_child(alt_so, a.reps, a.points))
        new.append(run_child(new_so, a.reps, a.points))
        print("round %d of %d measured" % (i + 1, a.rounds), file=sys.stderr, flush=True)
    rows = []
    for p in alt[0]:
        ma, mn = [r[p] for r in alt], [r[p] for r in new]
        margin = round(max(ma) - min(ma), 4)
        over = round(statistics.median(mn) - statistics.median(ma), 4)
        rows.append({"point": p, "alt_medians": ma, "new_medians": mn, "alt_median": statistics.median(ma),
                     "new_median": statistics.median(mn), "margin": margin, "new_minus_alt": over, "within": over <= margin})
        print(json.dumps(rows[-1]), flush=True)
    res["points"] = rows
    if a.bench:
        key = "bench_py_" + ("verify_cell_kzg_proof_batch_n8192" if a.points == "verify" else "recover_cells_and_kzg_proofs_batch256")
        res[key] = {"alt": bench_figure(alt_so, a.points), "new": bench_figure(new_so, a.points)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
