"""ckzg_hip_repair_cosets_and_kzg_proofs_rows on poisoned temporaries, in a process of its own
(tests/test_gpu_coset_repair.py starts it under tests/watchdog.py, the way tests/test_gpu_poison.py starts
tests/poison/driver.py):

    python tests/coset_repair_poison_driver.py CASES.pickle REPORT.json [FILLS]

(FILLS: the fill bytes of the runs, "0,255,1" unless given; "0,0,0" is how the time limit was measured.)

CASES: e -> rows, commitments, held proofs and what the oracle says must come back.  Every case runs three times in a row
on settings loaded for that run -- option "poison_temporaries" off, 0xFF, 0x01 -- into host buffers pre-filled with 0xA5.
The report is rewritten after every case; the child stops at the first C return it did not expect or the first HIP
error, starts nothing further on the GPU, and says where it was.  No retries."""
import ctypes as C
import hashlib
import json
import os
import pickle
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

A5 = 0xA5
SMALL_TABLES = {"commit_wbits": 8, "proof_wbits": 6, "fk20_wbits": 8}
POISONS = (0, 0xFF, 0x01)
NAME = "ckzg_hip_repair_cosets_and_kzg_proofs_rows"
EVALS = 8192 * 32


def one_case(k, e, case):
    """(fails, digest of everything the call wrote)"""
    rows, want = case["rows"], case["want"]
    nr, ps = len(rows), 48 * (8192 >> e)
    start = [0]
    for idx, _ in rows:
        start.append(start[-1] + len(idx))
    flat = [i for idx, _ in rows for i in idx]
    fill = lambda n: (C.c_char * n).from_buffer(bytearray([A5]) * n)
    ev, pr = fill(nr * EVALS), fill(nr * ps)
    st, vd = (C.c_uint8 * nr)(*([A5] * nr)), (C.c_uint8 * nr)(*([A5] * nr))
    ok, stats = (C.c_uint8 * len(flat))(*([A5] * len(flat))), (C.c_uint64 * 4)(*([A5] * 4))
    f = getattr(k.lib, NAME)
    f.restype = C.c_int
    ret = f(ev, pr, st, vd, ok, stats, (C.c_uint64 * len(flat))(*flat), b"".join(b for _, b in rows),
            (C.c_uint64 * (nr + 1))(*start), C.c_uint64(nr), b"".join(case["cms"]), b"".join(case["hp"]), C.c_uint32(e), k.sp)
    if ret != 0:
        raise RuntimeError("%s -> %d" % (NAME, ret))
    fails = []
    if list(vd) != want["vd"]:
        fails.append("verdicts %r" % list(vd))
    if list(st) != want["st"]:
        fails.append("status %r" % list(st))
    if [i for i, v in enumerate(ok) if v != 1] != want["bad_ok"] or any(v not in (0, 1) for v in ok):
        fails.append("coset_ok: not true at %r" % [i for i, v in enumerate(ok) if v != 1][:20])
    if list(stats)[:3] != want["stats"]:
        fails.append("stats %r" % list(stats))
    for r, exp in want["ev"].items():
        if ev.raw[r * EVALS:(r + 1) * EVALS] != exp:
            fails.append("evaluations of row %d" % r)
    for r, exp in want["pr"].items():
        if pr.raw[r * ps:(r + 1) * ps] != exp:
            fails.append("proofs of row %d" % r)
    h = hashlib.sha256()
    for r in sorted(want["ev"]):   # (an UNRECOVERABLE row's output is unspecified: left out)
        h.update(ev.raw[r * EVALS:(r + 1) * EVALS] + pr.raw[r * ps:(r + 1) * ps])
    h.update(bytes(st) + bytes(vd) + bytes(ok) + repr(list(stats)[:3]).encode())
    return fails, h.hexdigest()


def main(cases_path, report_path, fills=POISONS):
    from kzg_ctypes import HIP_SO, Kzg
    with open(cases_path, "rb") as f:
        cases = pickle.load(f)
    report = {"runs": {}, "digests": {}, "seconds": {}, "stopped": None, "done": False}

    def save():
        tmp = report_path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(report, f)
        os.replace(tmp, report_path)

    save()
    rt = C.CDLL("libamdhip64.so")
    lib = C.CDLL(HIP_SO)
    setopt = lib.ckzg_hip_set_option
    setopt.restype, setopt.argtypes = C.c_int, [C.c_char_p, C.c_int64]
    try:
        for poison in fills:
            key = "0x%02X" % poison
            report["runs"][key], report["digests"][key] = {}, {}
            where = "load"
            t0 = time.time()
            try:
                # settings of this run's own, loaded with the fill byte already set: the first case is a first call
                if setopt(b"poison_temporaries", poison) != 0:
                    raise RuntimeError("option poison_temporaries = %d refused" % poison)
                k = Kzg(HIP_SO, "", precompute=0, options=SMALL_TABLES)
                for e in sorted(cases):
                    where = "e = %d" % e
                    sys.stderr.write("[poison] coset repair %s %s\n" % (key, where))
                    sys.stderr.flush()
                    fails, digest = one_case(k, e, cases[e])
                    err = rt.hipDeviceSynchronize()
                    if err != 0:
                        raise RuntimeError("HIP error %d after the call" % err)
                    report["runs"][key][str(e)], report["digests"][key][str(e)] = fails, digest
                    save()
                k.close()
            except Exception as ex:   # nothing further on the GPU
                report["stopped"] = {"poison": key, "where": where, "why": "%s: %s" % (type(ex).__name__, ex)}
                save()
                return 1
            finally:
                report["seconds"][key] = round(time.time() - t0, 3)
        report["done"] = True
        save()
        return 0
    finally:
        if report["stopped"] is None:   # (after a stop the child makes no further call into the library: it ends)
            setopt(b"poison_temporaries", 0)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], tuple(int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else POISONS))
