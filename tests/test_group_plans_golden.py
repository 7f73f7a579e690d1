"""The job layouts of the two grouped verifications (csrc/group_jobs.hpp under csrc/cell_groups_plan.hpp and
csrc/blob_groups_plan.hpp) are, bit for bit, what they were before the layout was written once: for a fixed list of
shapes hs_cell_groups_replay and hs_blob_groups_replay run on seeded inputs, and a SHA-256 over info, term_src,
part_off and sc is compared with tests/golden/group_plans_parent.json.

The fixture is recorded from the libhost_shim.so of the commit BEFORE that change, never from the tree under test:
    python tests/test_group_plans_golden.py --record PATH_TO_THAT_SO OUT.json
Every shape runs twice: quad_max_terms large (four-lane form, jobs padded to 8 terms) and 0 (padded to 32)."""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys

from conftest import ROOT, SHIM_SO

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
GOLDEN = os.path.join(ROOT, "tests", "golden", "group_plans_parent.json")
CAP = 16384
QUAD_MAX = (1 << 20, 0)


def _le(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def _roots():
    w, x, out = pow(7, (R - 1) // 8192, R), 1, []
    for _ in range(8193):
        out.append(x)
        x = x * w % R
    return _le(out)


def _partitions(seed, count, lo, hi):
    """`count` partitions of lo..hi units into at most 40 groups, empty groups among them"""
    rnd = random.Random(seed)
    out = []
    for _ in range(count):
        G = rnd.randrange(1, 41)
        N = rnd.randrange(lo, hi + 1)
        cuts = sorted(rnd.randrange(0, N + 1) for _ in range(G - 1))
        out.append([b - a for a, b in zip([0] + cuts, cuts + [N])])
    return out


SHARED = {"one_unit": [1], "empty_first": [0, 2, 3], "empty_middle": [2, 0, 0, 3], "empty_last": [3, 2, 0], "all_empty": [0, 0, 0]}


def blob_cases():
    """name -> group sizes"""
    cases = dict(SHARED)
    cases["groups_1_2_3"] = [1, 2, 3]
    for n in (3, 4, 7, 8, 15, 16, 31, 32):
        cases["n%d" % n] = [n]
    cases["n_mixed"] = [3, 4, 7, 8, 15, 16, 31, 32]
    cases["four_of_3"] = [3, 3, 3, 3]   # 64 terms in the quad form; [3] alone is 64 terms when padded to 32, [16] is 96
    for i, sizes in enumerate(_partitions(4844, 30, 0, 200)):
        cases["random%02d" % i] = sizes
    return cases


def cell_cases():
    """name -> groups of (commitment id, column) cells"""
    seq = lambda n, c0=0: [(0, (c0 + j) % 128) for j in range(n)]
    cases = {k: [seq(n, 5 * i) for i, n in enumerate(v)] for k, v in SHARED.items()}
    cases["one_cell_per_group"] = [[(g % 2, 9 * g)] for g in range(5)]
    cases["one_commitment"] = [[(0, c) for c in (3, 5, 8, 13, 21, 34)]]
    cases["own_commitments"] = [[(j, 2 * j + 1) for j in range(6)]]
    cases["commitment_across_groups"] = [[(0, 1), (1, 2)], [(1, 2), (2, 3), (0, 4)], [(2, 1)]]
    cases["repeated_columns"] = [[(0, 7), (1, 7), (0, 7), (0, 9), (1, 9)], [(1, 7), (1, 7)]]
    cases["cells_64"] = [[(j % 3, j) for j in range(64)]]
    cases["cells_65"] = [[(j % 3, (2 * j) % 128) for j in range(65)], [(0, 0)]]
    cases["columns_0_127"] = [[(0, 0), (0, 127)], [(1, 127), (0, 0), (1, 0)]]
    rnd = random.Random(7594)
    # (the replay costs 4096 field products per aggregated column: most partitions small, one of them large)
    for i, sizes in enumerate(_partitions(7594, 24, 0, 24) + _partitions(7595, 1, 150, 200)):
        nc = rnd.randrange(1, 9)
        cases["random%02d" % i] = [[(rnd.randrange(nc), rnd.randrange(128)) for _ in range(n)] for n in sizes]
    return cases


def _digest(info, src, part_off, sc, total, G):
    h = hashlib.sha256()
    h.update(bytes(info))
    h.update(bytes(src)[:4 * total])
    h.update(bytes(part_off)[:4 * (2 * G + 1)])
    h.update(bytes(sc)[:32 * total])
    return h.hexdigest()


def digests(lib):
    """{plan/case/quad_max: sha256} of every shape, through the shim `lib`"""
    lib.hs_cell_groups_replay.restype = C.c_long
    lib.hs_blob_groups_replay.restype = C.c_long
    sc, src = (C.c_uint32 * (CAP * 8))(), (C.c_uint32 * CAP)()
    roots = _roots()
    out = {}
    for name, sizes in blob_cases().items():
        G, N = len(sizes), sum(sizes)
        start = (C.c_uint64 * (G + 1))(*[sum(sizes[:g]) for g in range(G + 1)])
        rnd = random.Random("blob/" + name)
        z, y, r = (_le(rnd.randrange(R) for _ in range(n)) for n in (N, N, G))
        for quad_max in QUAD_MAX:
            part_off, info = (C.c_uint32 * (2 * G + 1))(), (C.c_uint32 * 2)()
            total = lib.hs_blob_groups_replay(sc, src, part_off, info, C.c_size_t(CAP), start, C.c_size_t(G), z, y, r,
                                              C.c_size_t(quad_max))
            assert total >= 0 and total % 64 == 0 and info[0] == total, (name, total)
            out["blob/%s/%d" % (name, quad_max)] = _digest(info, src, part_off, sc, total, G)
    for name, groups in cell_cases().items():
        flat = [c for g in groups for c in g]
        G, N = len(groups), len(flat)
        start = (C.c_uint64 * (G + 1))(*[sum(len(g) for g in groups[:k]) for k in range(G + 1)])
        # chunk-wide commitment ids in order of first appearance, as the call numbers them
        ids = {}
        commit = (C.c_uint32 * N)(*[ids.setdefault(c[0], len(ids)) for c in flat])
        cols = (C.c_uint64 * N)(*[c[1] for c in flat])
        rnd = random.Random("cell/" + name)
        cells, r = _le(rnd.randrange(R) for _ in range(64 * N)), _le(rnd.randrange(R) for _ in range(G))
        for quad_max in QUAD_MAX:
            part_off, info = (C.c_uint32 * (2 * G + 1))(), (C.c_uint32 * 4)()
            total = lib.hs_cell_groups_replay(sc, src, part_off, info, C.c_size_t(CAP), start, C.c_size_t(G), commit,
                                              C.c_size_t(len(ids)), cols, cells, r, roots, C.c_size_t(quad_max))
            assert total >= 0 and total % 64 == 0 and info[0] == total, (name, total)
            out["cell/%s/%d" % (name, quad_max)] = _digest(info, src, part_off, sc, total, G)
    return out


def test_totals_of_the_blob_shapes_cover_both_sides_of_64():
    """(the arithmetic the shape list relies on: jobs of 2 n + 1 and n terms, each padded to 8 or to 32)"""
    pad = lambda n, per: (n + per - 1) // per * per
    total = lambda sizes, per: sum(pad(2 * n + 1, per) + pad(n, per) for n in sizes if n)
    assert total([3, 3, 3, 3], 8) % 64 == 0 and total([3], 8) % 64 != 0
    assert total([3], 32) % 64 == 0 and total([16], 32) % 64 != 0


def test_plans_are_bit_identical_to_the_recorded_ones():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    want = json.load(open(GOLDEN))
    got = digests(C.CDLL(SHIM_SO))
    assert sorted(got) == sorted(want), "the shape list and the fixture differ: record the fixture again from the parent's shim"
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, differ


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    with open(sys.argv[3], "w") as f:
        json.dump(digests(C.CDLL(os.path.abspath(sys.argv[2]))), f, indent=0, sort_keys=True)
        f.write("\n")
