"""ckzg_hip_compute_domain_kzg_proofs_batch (a blob opened at every point of the evaluation domain in one call) at the
C-ABI, against what a client had before it: ckzg_hip_compute_kzg_proof_batch over the same blobs at their 4096 domain
points each, on another build of the library (the parent commit's) loaded in the same process.

    python tools/bench_domain_openings.py --alt PATH/libckzg_hip.so [--out FILE] [--sizes 1,4,16,64] [--reps 20]

Per size: one warm-up and `reps` timed calls of the new call, then the alternative alternating with further calls of the
new one (`reps` times at one blob, fewer above: it takes 80 ms per blob); median and minimum of the wall time, both calls
end in a device synchronise.  Above --alt-max blobs only the new call runs: the alternative's input is 512 MB per blob.
`wins` is the README's standard: the new call's median below the alternative's minimum.  The outputs of both calls are
compared byte for byte at every size where both run.  Also: the first call on fresh settings against the second (the
lazy transformed setup and its bytes) and ckzg_hip_g1_fft alone at n = 8192 with 1 and 16 transforms (host conversions
included: it is a host-pointer call).  Prints one JSON object (and writes it to FILE)."""
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
PER = 4096 * 48


def fr(v):
    return (v % R).to_bytes(32, "big")


def brp(i, bits=12):
    return int(format(i, "0%db" % bits)[::-1], 2)


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alt", required=True, help="the other build of libckzg_hip.so (the parent commit's)")
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--alt-max", type=int, default=16, help="largest size at which the alternative is run (512 MB of input per blob)")
    a = ap.parse_args()
    mod = ge.load_package()
    rnd = random.Random(1)
    blobs = [b"".join(fr(rnd.randrange(R)) for _ in range(4096)) for _ in range(4)]
    w = pow(7, (R - 1) // 4096, R)
    domain = b"".join(fr(pow(w, brp(j), R)) for j in range(4096))
    res = {"tool": "bench_domain_openings", "reps": a.reps, "unit": "ms"}

    # the first call on fresh settings builds the transformed setup; the second does not
    hip = mod.Kzg(mod.HIP_SO)
    f = hip.lib.ckzg_hip_compute_domain_kzg_proofs_batch
    f.restype = C.c_int
    out1, st1 = C.create_string_buffer(PER), (C.c_uint8 * 1)()
    first = ms(lambda: f(out1, st1, blobs[0], C.c_uint64(1), hip.sp))
    second = ms(lambda: f(out1, st1, blobs[0], C.c_uint64(1), hip.sp))
    res["lazy_state"] = {"first_call_ms": round(first, 3), "second_call_ms": round(second, 3),
                         "xhat_bytes": 8192 * 96, "twiddle_record_bytes": 8192 * 32}
    alt = mod.Kzg(a.alt)
    g = alt.lib.ckzg_hip_compute_kzg_proof_batch
    g.restype = C.c_int
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        bb = b"".join(blobs[i % len(blobs)] for i in range(n))
        out, st = C.create_string_buffer(PER * n), (C.c_uint8 * n)()
        def new():
            assert f(out, st, bb, C.c_uint64(n), hip.sp) == 0
        new()   # warm-up: arena, code objects
        tn = [ms(new) for _ in range(a.reps)]
        row = {"blobs": n, "new_median": round(statistics.median(tn), 3), "new_min": round(min(tn), 3),
               "new_per_blob": round(statistics.median(tn) / n, 3)}
        if n <= a.alt_max:
            # the alternative: every blob 4096 times (512 MB each), next to the 4096 points
            items = 4096 * n
            rep_blobs = b"".join(blobs[i % len(blobs)] * 4096 for i in range(n))
            zs = domain * n
            pr, ys, st2 = C.create_string_buffer(48 * items), C.create_string_buffer(32 * items), (C.c_uint8 * items)()

            def old():
                assert g(pr, ys, st2, rep_blobs, zs, C.c_uint64(items), alt.sp) == 0
            old()
            assert out.raw == pr.raw, "the two calls disagree at n = %d" % n
            reps_old = a.reps if n == 1 else max(3, a.reps // n)
            to = []
            for _ in range(reps_old):   # alternating with the new call, whose time is taken again next to it
                to.append(ms(old))
                tn.append(ms(new))
            row.update({"new_median": round(statistics.median(tn), 3), "new_min": round(min(tn), 3),
                        "new_per_blob": round(statistics.median(tn) / n, 3),
                        "alt_median": round(statistics.median(to), 3), "alt_min": round(min(to), 3), "alt_reps": reps_old,
                        "alt_input_bytes": len(rep_blobs) + len(zs)})
            row["wins"] = row["new_median"] < row["alt_min"]
            row["alt_min_over_new_median"] = round(row["alt_min"] / row["new_median"], 2)
            del rep_blobs, zs, pr, ys
        else:
            row["alt"] = "not measured: its input would be %d bytes of repeated blobs" % (n * 4096 * 131072)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res["sizes"] = rows

    # the transform alone: 8192 points in, 8192 out, through the host-pointer call
    fft = hip.lib.ckzg_hip_g1_fft
    fft.restype = C.c_int
    gen48 = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
    res["g1_fft_8192"] = []
    # inputs: the transform of a delta at index 1 is [w^k]G, 8192 distinct subgroup points with Z != 1
    gen = C.create_string_buffer(144)
    orc = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    aff = C.create_string_buffer(96)
    assert orc.og1_uncompress(aff, gen48) == 0
    orc.og1_from_affine(gen, aff)
    seed = C.create_string_buffer(8192 * 144)
    assert fft(seed, bytes(144) + gen.raw + bytes(144 * 8190), C.c_uint64(8192), C.c_uint64(1), 0, hip.sp) == 0
    for count in (1, 16):
        src, dst = seed.raw * count, C.create_string_buffer(8192 * 144 * count)

        def run():
            assert fft(dst, src, C.c_uint64(8192), C.c_uint64(count), 0, hip.sp) == 0
        run()
        t = [ms(run) for _ in range(a.reps)]
        res["g1_fft_8192"].append({"count": count, "median": round(statistics.median(t), 3), "min": round(min(t), 3)})
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    hip.close()
    alt.close()


if __name__ == "__main__":
    main()
