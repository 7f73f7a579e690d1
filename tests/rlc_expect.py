"""What the scalar vectors of the batch checks must hold, as Python integers: the weights r^i of a random linear
combination and the products and sums made from them, laid out term by term the way csrc/group_jobs.hpp,
csrc/blob_groups_plan.hpp and csrc/coset_groups_plan.hpp (at cosets of 64) document it.  Nothing here reads the library under test.
Shared by tests/test_gpu_rlc_stages.py (the device stages) and the CPU replay tests (tests/test_blob_groups_cpu.py,
tests/test_cell_groups_cpu.py)."""
import random

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NO_POINT = 0xffffffff
# a group of one (needs no challenge), an empty one, one cell past a wave, two, a whole wave, two waves and two, one
# short of a wave, three
GROUP_SIZES = [1, 0, 65, 2, 64, 130, 63, 3]


def challenges(seed):
    """0, 1, 2, R - 1 and two random values"""
    rnd = random.Random(seed)
    return [0, 1, 2, R - 1, rnd.randrange(3, R - 1), rnd.randrange(3, R - 1)]


def group_challenges(seed, ngroups=len(GROUP_SIZES)):
    """one value per group; the groups of 65 and of 130 get 0 and 1, the others random values, R - 1 and 2"""
    rnd = random.Random(seed)
    rs = [rnd.randrange(3, R - 1) for _ in range(ngroups)]
    if ngroups == len(GROUP_SIZES):
        rs[2], rs[5], rs[4], rs[6] = 0, 1, R - 1, 2
    return rs


def roots_of_unity():
    """w^i, i <= 8192, for w = 7^((R - 1) / 8192)"""
    w = pow(7, (R - 1) // 8192, R)
    out, x = [], 1
    for _ in range(8193):
        out.append(x)
        x = x * w % R
    assert out[8192] == 1 and out[4096] == R - 1
    return out


def brev7(c):
    return int("{:07b}".format(c & 127)[::-1], 2)


def coset_factor(roots, col):
    """h_k^64 of column col: w^(64 brev7(col))"""
    return roots[64 * brev7(col)]


def le32(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def from_le32(buf, n):
    raw = bytes(buf)
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]


def _pad(src, sc, per):
    while len(src) % per:
        src.append(NO_POINT)
        sc.append(0)


def blob_group_terms(sizes, z, y, rs, per):
    """(term_src, scalars, part_off) of the jobs A_0, B_0, A_1, ... over the pool [N commitments | N proofs | G]:
    A_g = [C_a .. | proof_a .. | G] with r^(i-a), r^(i-a) z_i, -sum r^(i-a) y_i; B_g = [proof_a ..] with r^(i-a)"""
    n_all = sum(sizes)
    src, sc, part_off = [], [], []
    a = 0
    for g, n in enumerate(sizes):
        pw = [pow(rs[g], i, R) for i in range(n)]
        for job in (0, 1):
            part_off.append(len(src) // per)
            if n and job == 0:
                src += [a + i for i in range(n)]
                sc += pw
                src += [n_all + a + i for i in range(n)]
                sc += [pw[i] * z[a + i] % R for i in range(n)]
                src.append(2 * n_all)
                sc.append(-sum(pw[i] * y[a + i] for i in range(n)) % R)
            elif n:
                src += [n_all + a + i for i in range(n)]
                sc += pw
            _pad(src, sc, per)
        a += n
    part_off.append(len(src) // per)
    _pad(src, sc, 64)
    return src, sc, part_off


def cell_group_terms(sizes, cell_commit, num_commits, cols, rs, roots, per):
    """(term_src, scalars, part_off) over the pool [N proofs | the chunk's distinct commitments | 64 setup points]:
    A_g = [the group's commitments, in order of first appearance | its proofs | 64 setup points] with the sums of
    r^(i-a) over the cells that name each commitment, r^(i-a) h_k^64, and the negated interpolation coefficients
    (None here: not a weight); B_g = [its proofs] with r^(i-a)"""
    n_all = sum(sizes)
    src, sc, part_off = [], [], []
    a = 0
    for g, n in enumerate(sizes):
        pw = [pow(rs[g], i, R) for i in range(n)]
        for job in (0, 1):
            part_off.append(len(src) // per)
            if n and job == 0:
                order = []
                for i in range(n):
                    if cell_commit[a + i] not in order:
                        order.append(cell_commit[a + i])
                for cm in order:
                    src.append(n_all + cm)
                    sc.append(sum(pw[i] for i in range(n) if cell_commit[a + i] == cm) % R)
                src += [a + i for i in range(n)]
                sc += [pw[i] * coset_factor(roots, cols[a + i]) % R for i in range(n)]
                src += [n_all + num_commits + k for k in range(64)]
                sc += [None] * 64
            elif n:
                src += [a + i for i in range(n)]
                sc += pw
            _pad(src, sc, per)
        a += n
    part_off.append(len(src) // per)
    _pad(src, sc, 64)
    return src, sc, part_off


def check_terms(got_src, got_sc, got_part_off, want, unpinned=None):
    """term by term; a term whose expected scalar is None must equal `unpinned` if that is given"""
    src, sc, part_off = want
    assert list(got_part_off) == part_off
    assert len(got_src) == len(src) and list(got_src) == src
    for t, (g, w) in enumerate(zip(got_sc, sc)):
        if w is None:
            if unpinned is not None:
                assert g == unpinned, "term %d" % t
        else:
            assert g == w, "term %d (point %d): %x, expected %x" % (t, src[t], g, w)
