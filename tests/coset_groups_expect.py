"""The model of ckzg_hip_verify_coset_kzg_proof_batch_groups in Python integers: the job layout of
csrc/coset_groups_plan.hpp with every scalar, the interpolation terms included, and the stage values the GPU stage tests
compare with.  A chunk is described by `sizes` (items per group), and per item its chunk-wide commitment id, its coset
and its l = 2^e values; `rs` are the groups' challenges.

Two routes to the interpolation terms, compared in tests/test_coset_groups_cpu.py: item by item through
coset_verify_expect.interp_coeffs (group_terms), and the device's -- aggregate each (group, coset) row first, transform
it, take the coset factor out, add the rows of a group (rows_of, rows_interp, group_interp)."""
import coset_verify_expect as cx
from domain_expect import R

NO_POINT = 0xffffffff


def roots8193():
    """w^i, i <= 8192, as the shims take them"""
    return cx.roots() + [1]


def _pad(src, sc, per):
    while len(src) % per:
        src.append(NO_POINT)
        sc.append(0)


def powers(sizes, rs):
    """r_g^(i - start_g) per item"""
    return [pow(rs[g], i, R) for g, n in enumerate(sizes) for i in range(n)]


def group_terms(sizes, item_commit, num_commits, cols, values, rs, e, per):
    """(term_src, scalars, part_off) over the pool [N proofs | the chunk's distinct commitments | l setup points]:
    A_g = [the group's commitments, in order of first appearance | its proofs | l setup points] with the sums of r^(i-a)
    over the items that name each commitment, r^(i-a) x_c^l, and minus the sum over the items of r^(i-a) times the
    item's interpolation coefficients; B_g = [its proofs] with r^(i-a).  Padded to `per` per job and to 64 in all."""
    l, rt, n_all = 1 << e, cx.roots(), sum(sizes)
    src, sc, part_off = [], [], []
    a = 0
    for g, n in enumerate(sizes):
        pw = [pow(rs[g], i, R) for i in range(n)]
        for job in (0, 1):
            part_off.append(len(src) // per)
            if n and job == 0:
                order = []
                for i in range(n):
                    if item_commit[a + i] not in order:
                        order.append(item_commit[a + i])
                for cm in order:
                    src.append(n_all + cm)
                    sc.append(sum(pw[i] for i in range(n) if item_commit[a + i] == cm) % R)
                src += [a + i for i in range(n)]
                sc += [pw[i] * rt[cx.shift_root(cols[a + i], e)] % R for i in range(n)]
                interp = [0] * l
                for i in range(n):
                    for k, ak in enumerate(cx.interp_coeffs(values[a + i], cols[a + i], e)):
                        interp[k] = (interp[k] + pw[i] * ak) % R
                src += [n_all + num_commits + k for k in range(l)]
                sc += [-v % R for v in interp]
            elif n:
                src += [a + i for i in range(n)]
                sc += pw
            _pad(src, sc, per)
        a += n
    part_off.append(len(src) // per)
    _pad(src, sc, 64)
    return src, sc, part_off


def rows_of(sizes, cols):
    """the distinct (group, coset) pairs in order of first appearance: (row_group, row_col, row of each item)"""
    row_grp, row_col, item_row = [], [], []
    a = 0
    for g, n in enumerate(sizes):
        seen = {}
        for i in range(a, a + n):
            if cols[i] not in seen:
                seen[cols[i]] = len(row_col)
                row_grp.append(g)
                row_col.append(cols[i])
            item_row.append(seen[cols[i]])
        a += n
    return row_grp, row_col, item_row


def rows_aggregate(sizes, cols, values, rp, e):
    """rows[t l + j] = sum over the items i of row t of rp[i] y_i[j]"""
    l = 1 << e
    _, row_col, item_row = rows_of(sizes, cols)
    rows = [0] * (len(row_col) * l)
    for i, t in enumerate(item_row):
        for j in range(l):
            rows[t * l + j] = (rows[t * l + j] + rp[i] * values[i][j]) % R
    return rows


def rows_interp(rows, row_col, e):
    """each row's coefficients over the l-th roots of unity, coefficient k times x_c^-k of the row's coset"""
    l, rt = 1 << e, cx.roots()
    out = []
    for t, c in enumerate(row_col):
        co = cx.column_coeffs(rows[t * l:(t + 1) * l], e)
        out += [co[k] * rt[cx.unshift_root(c, e, k)] % R for k in range(l)]
    return out


def group_interp(rows, row_grp, ngroups, e):
    """per group the sum of its rows"""
    l = 1 << e
    out = [[0] * l for _ in range(ngroups)]
    for t, g in enumerate(row_grp):
        for k in range(l):
            out[g][k] = (out[g][k] + rows[t * l + k]) % R
    return out


def setup_terms(sizes, item_commit, e, per):
    """first term of the l setup points of A_g, None for an empty group"""
    l = 1 << e
    out, at, a = [], 0, 0
    for n in sizes:
        if not n:
            out.append(None)
        else:
            nc = len(set(item_commit[a:a + n]))
            out.append(at + nc + n)
            at += -(-(nc + n + l) // per) * per + -(-n // per) * per
        a += n
    return out
