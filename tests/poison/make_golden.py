"""Writes tests/golden/poison_openings_b{0,1}.bin: for the two blobs corpus.blob(0) and corpus.blob(1) their 8192
openings of coset size one -- compute_kzg_proof of the CPU oracle at every point of the extended domain, one call per
point -- followed by their 1024 multiproofs of coset size 8, made from those by three steps of
pi_e[c] = [1 / (2a)] (pi_{e-1}[2c] - pi_{e-1}[2c+1]), a = x_c^(l/2), in the oracle's G1 arithmetic.  The library under
test takes no part.  Some minutes on eight cores; tests/test_gpu_poison.py (its CPU test) re-derives sampled entries.

    python tests/poison/make_golden.py [PROCESSES]
"""
import ctypes as C
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import corpus  # noqa: E402

_orc = None


def _proofs(job):
    global _orc
    which, lo, hi = job
    if _orc is None:
        _orc = corpus.load_oracle()
    blob = corpus.blob(which)
    out = []
    for j in range(lo, hi):
        proof, y = _orc.compute_kzg_proof(blob, corpus.EXT[j])
        out.append(proof)
    return which, lo, b"".join(out)


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    step = 128
    jobs = [(w, lo, lo + step) for w in (0, 1) for lo in range(0, 8192, step)]
    size_one = {0: bytearray(8192 * 48), 1: bytearray(8192 * 48)}
    with multiprocessing.Pool(procs) as pool:
        for which, lo, raw in pool.imap_unordered(_proofs, jobs):
            size_one[which][48 * lo:48 * lo + len(raw)] = raw
            sys.stderr.write("blob %d: %d..%d\n" % (which, lo, lo + step))
    g1 = corpus.OracleG1()
    for which in (0, 1):
        level = [bytes(size_one[which][48 * j:48 * j + 48]) for j in range(8192)]
        for e in (1, 2, 3):
            level = corpus.ladder(g1, level, e)
        path = corpus.golden_path(which)
        with open(path, "wb") as f:
            f.write(bytes(size_one[which]) + b"".join(level))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
