"""ckzg_hip_compute_coset_kzg_proofs_batch (a blob opened on every coset of 2^e points of the extended domain in one
call) at the C-ABI, every e = 0 .. 6 at 1 / 4 / 16 blobs, default tables, and at the two ends what a client had before
it, on another build of the library (the parent commit's) loaded in the same process:

    e = 0   ckzg_hip_compute_kzg_proof_batch over the blob repeated at all 8192 points (1 GB of input per blob), at 1
            and 4 blobs; with --outer-only the 4096 outer points that way plus ckzg_hip_compute_domain_kzg_proofs_batch
    e = 6   ckzg_hip_compute_cells_and_kzg_proofs_batch (cells and proofs), at every size

    python tools/bench_coset_openings.py --alt PATH/libckzg_hip.so [--out FILE] [--sizes 1,4,16] [--reps 20] [--outer-only]

Per (e, size): one warm-up and `reps` timed calls with evals wanted; median and minimum of the wall time, every call ends
in a device synchronise.  Where an alternative runs it alternates with further calls of the new one, and both outputs
are compared byte for byte.  `wins` is the README's standard: the new call's median below the alternative's minimum.
The sizes in between have no alternative in the library and are reported as they are.  Also: per e the first call on
fresh settings against the second (the lazy transformed setup).  Prints one JSON object (and writes it to FILE)."""
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
BLOB = 131072
EV = 8192 * 32


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
    ap.add_argument("--alt", required=True, help="the other build of libckzg_hip.so (the parent commit's)")
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="1,4,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--alt-max", type=int, default=4, help="largest size at which the e = 0 alternative is run")
    ap.add_argument("--outer-only", action="store_true",
                    help="e = 0 alternative: the 4096 outer points plus the domain call (512 MB of input per blob, not 1 GB)")
    a = ap.parse_args()
    mod = ge.load_package()
    rnd = random.Random(1)
    blobs = [b"".join(fr(rnd.randrange(R)) for _ in range(4096)) for _ in range(4)]
    w = pow(7, (R - 1) // 8192, R)
    pw = [1] * 8192
    for i in range(1, 8192):
        pw[i] = pw[i - 1] * w % R
    ext = b"".join(fr(pw[brp(j, 13)]) for j in range(8192))
    sizes = [int(x) for x in a.sizes.split(",")]
    res = {"tool": "bench_coset_openings", "reps": a.reps, "unit": "ms", "tables": "default", "evals": True,
           "e0_alternative": "outer 4096 points + domain call" if a.outer_only else "all 8192 points in one call"}

    # per e: the first call on fresh settings builds that size's transformed setup; the second does not
    lazy = []
    for e in range(7):
        k = mod.Kzg(mod.HIP_SO)
        f = k.lib.ckzg_hip_compute_coset_kzg_proofs_batch
        f.restype = C.c_int
        out, ev, st = C.create_string_buffer((8192 >> e) * 48), C.create_string_buffer(EV), (C.c_uint8 * 1)()
        call = lambda: f(out, ev, st, blobs[0], C.c_uint64(1), C.c_uint32(e), k.sp)
        first, second = ms(call), ms(call)
        lazy.append({"log2_coset": e, "first_call_ms": round(first, 3), "second_call_ms": round(second, 3)})
        k.close()
    res["lazy_state"] = {"xhat_bytes_per_size": 8192 * 96, "calls": lazy}

    hip, alt = mod.Kzg(mod.HIP_SO), mod.Kzg(a.alt)
    f = hip.lib.ckzg_hip_compute_coset_kzg_proofs_batch
    g_point, g_dom, g_cells = (getattr(alt.lib, n) for n in (
        "ckzg_hip_compute_kzg_proof_batch", "ckzg_hip_compute_domain_kzg_proofs_batch", "ckzg_hip_compute_cells_and_kzg_proofs_batch"))
    for fn in (f, g_point, g_dom, g_cells):
        fn.restype = C.c_int
    rows = []
    for e in range(7):
        m = 8192 >> e
        for n in sizes:
            bb = b"".join(blobs[i % len(blobs)] for i in range(n))
            out, ev, st = C.create_string_buffer(m * 48 * n), C.create_string_buffer(EV * n), (C.c_uint8 * n)()

            def new():
                assert f(out, ev, st, bb, C.c_uint64(n), C.c_uint32(e), hip.sp) == 0
            new()   # warm-up: arena, code objects, this size's setup
            tn = [ms(new) for _ in range(a.reps)]
            row = {"log2_coset": e, "blobs": n, "proofs_per_blob": m}
            old = None
            if e == 0 and n <= a.alt_max:
                per = 4096 if a.outer_only else 8192
                items = per * n
                rep_blobs = b"".join(blobs[i % len(blobs)] * per for i in range(n))
                zs = (ext[4096 * 32:] if a.outer_only else ext) * n
                pr, ys, st2 = C.create_string_buffer(48 * items), C.create_string_buffer(32 * items), (C.c_uint8 * items)()
                dom = C.create_string_buffer(4096 * 48 * n)

                def old():
                    assert g_point(pr, ys, st2, rep_blobs, zs, C.c_uint64(items), alt.sp) == 0
                    if a.outer_only:
                        assert g_dom(dom, st2, bb, C.c_uint64(n), alt.sp) == 0
                old()
                if a.outer_only:
                    want = b"".join(dom.raw[4096 * 48 * i:4096 * 48 * (i + 1)] + pr.raw[4096 * 48 * i:4096 * 48 * (i + 1)] for i in range(n))
                    assert ev.raw == b"".join(bb[BLOB * i:BLOB * (i + 1)] + ys.raw[BLOB * i:BLOB * (i + 1)] for i in range(n))
                else:
                    want = pr.raw
                    assert ev.raw == ys.raw, "the evaluations disagree at e = 0, n = %d" % n
                assert out.raw == want, "the two calls disagree at e = 0, n = %d" % n
                row["alt"] = "ckzg_hip_compute_kzg_proof_batch" + (" (outer points) + ckzg_hip_compute_domain_kzg_proofs_batch" if a.outer_only else "")
                row["alt_input_bytes"] = len(rep_blobs) + len(zs)
            elif e == 6:
                cells, pr = C.create_string_buffer(EV * n), C.create_string_buffer(128 * 48 * n)

                def old():
                    assert g_cells(cells, pr, st, bb, C.c_uint64(n), alt.sp) == 0
                old()
                assert out.raw == pr.raw and ev.raw == cells.raw, "the two calls disagree at e = 6, n = %d" % n
                row["alt"] = "ckzg_hip_compute_cells_and_kzg_proofs_batch"
            if old:
                reps_old = a.reps if e == 6 or n == 1 else max(3, a.reps // n)
                to = []
                for _ in range(reps_old):   # alternating with the new call, whose time is taken again next to it
                    to.append(ms(old))
                    tn.append(ms(new))
                row["alt_median"], row["alt_min"] = stats(to)
                row["alt_reps"] = reps_old
            row["new_median"], row["new_min"] = stats(tn)
            row["new_per_blob"] = round(row["new_median"] / n, 3)
            if old:
                row["wins"] = row["new_median"] < row["alt_min"]
                row["alt_min_over_new_median"] = round(row["alt_min"] / row["new_median"], 3)
                old = None
            rep_blobs = zs = pr = ys = dom = cells = None   # (gigabytes at e = 0)
            rows.append(row)
            print(json.dumps(row), flush=True)
    res["sizes"] = rows
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    hip.close()
    alt.close()


if __name__ == "__main__":
    main()
