"""The two openings calls, ckzg_hip_compute_domain_kzg_proofs_batch and ckzg_hip_compute_coset_kzg_proofs_batch, on two
builds of the library loaded in one process: this tree's and another (the parent commit's).  For a change that must
leave both calls as fast as they were.

    python tools/bench_openings_ab.py --alt PATH/libckzg_hip.so [--out FILE] [--reps 20] [--blocks 3]

Points: the domain call at 1, 4 and 16 blobs; the coset call at e = 0, 3, 6 at 1 and 4 blobs with evals wanted.  Per
point and block: one warm-up call of each build, then `reps` timed calls of each, alternating alt, new, alt, new ...;
the median of the wall time (every call ends in a device synchronise).  The whole block runs `blocks` times.  The margin
of a point is the spread of the alternative's own block medians, maximum minus minimum; `within` says whether the median
of the new build's block medians exceeds that of the alternative's by no more than the margin.  The outputs of both
builds are compared byte for byte at every point.  Also the first call on fresh settings (the lazy transformed setup) of
the domain call and of e = 3, on both builds.  Prints one JSON object (and writes it to FILE)."""
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
EV = 8192 * 32
POINTS = [("domain", None, n) for n in (1, 4, 16)] + [("coset", e, n) for e in (0, 3, 6) for n in (1, 4)]


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def check(ret):
    assert ret == 0, ret


def caller(k, kind, e, n, bb):
    """(call, outputs) of one point on the settings k"""
    if kind == "domain":
        f = k.lib.ckzg_hip_compute_domain_kzg_proofs_batch
        f.restype = C.c_int
        bufs = [C.create_string_buffer(4096 * 48 * n), (C.c_uint8 * n)()]
        return (lambda: check(f(bufs[0], bufs[1], bb, C.c_uint64(n), k.sp))), bufs
    f = k.lib.ckzg_hip_compute_coset_kzg_proofs_batch
    f.restype = C.c_int
    bufs = [C.create_string_buffer((8192 >> e) * 48 * n), C.create_string_buffer(EV * n), (C.c_uint8 * n)()]
    return (lambda: check(f(bufs[0], bufs[1], bufs[2], bb, C.c_uint64(n), C.c_uint32(e), k.sp))), bufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alt", required=True, help="the other build of libckzg_hip.so (the parent commit's)")
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    a = ap.parse_args()
    mod = ge.load_package()
    rnd = random.Random(1)
    blobs = [b"".join((rnd.randrange(R)).to_bytes(32, "big") for _ in range(4096)) for _ in range(4)]
    res = {"tool": "bench_openings_ab", "reps": a.reps, "blocks": a.blocks, "unit": "ms", "tables": "default",
           "alt": "the parent commit's build", "new": "this tree's build"}

    # the first call on fresh settings builds the transformed setup of its coset size
    first = []
    for kind, e in (("domain", None), ("coset", 3)):
        row = {"call": kind, "log2_coset": e}
        for name, so in (("alt", a.alt), ("new", mod.HIP_SO), ("alt_again", a.alt), ("new_again", mod.HIP_SO)):
            k = mod.Kzg(so)
            call, _ = caller(k, kind, e, 1, blobs[0])
            row[name + "_first_call_ms"] = round(ms(call), 3)
            row[name + "_second_call_ms"] = round(ms(call), 3)
            k.close()
        first.append(row)
        print(json.dumps(row), flush=True)
    res["first_call"] = first

    new, alt = mod.Kzg(mod.HIP_SO), mod.Kzg(a.alt)
    med = {p: {"alt": [], "new": []} for p in POINTS}
    for _ in range(a.blocks):
        for p in POINTS:
            kind, e, n = p
            bb = b"".join(blobs[i % len(blobs)] for i in range(n))
            (ca, oa), (cn, on) = caller(alt, kind, e, n, bb), caller(new, kind, e, n, bb)
            ca(), cn()   # warm-up: arena, code objects, this size's setup
            assert [bytes(x) for x in oa] == [bytes(x) for x in on], "the two builds disagree at %s" % (p,)
            ta, tn = [], []
            for _ in range(a.reps):
                ta.append(ms(ca))
                tn.append(ms(cn))
            med[p]["alt"].append(round(statistics.median(ta), 3))
            med[p]["new"].append(round(statistics.median(tn), 3))
    rows = []
    for p in POINTS:
        kind, e, n = p
        ma, mn = med[p]["alt"], med[p]["new"]
        margin = round(max(ma) - min(ma), 3)
        over = round(statistics.median(mn) - statistics.median(ma), 3)
        rows.append({"call": kind, "log2_coset": e, "blobs": n, "alt_block_medians": ma, "new_block_medians": mn,
                     "alt_median": statistics.median(ma), "new_median": statistics.median(mn), "margin": margin,
                     "new_minus_alt": over, "within": over <= margin, "outputs_equal": True})
        print(json.dumps(rows[-1]), flush=True)
    res["points"] = rows
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    new.close()
    alt.close()


if __name__ == "__main__":
    main()
