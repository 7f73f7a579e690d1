"""The model of ckzg_hip_verify_coset_kzg_proof_batch: the check of a multiproof on a coset of l = 2^e points of the
2N-point extended domain, in Python integers with a KNOWN secret s and scalars in place of points ([a]G is written a, so
e(A, [1]_2) = e(B, [s^l]_2) reads A = B s^l).  Four things, each checked by a second route in
tests/test_coset_verify_expect_cpu.py:

    the interpolation coefficients   a_k = x_c^-k (1/l) sum_j y_j w_l^(-brp_e(j) k)
    the identity of one item         C - I(s) + x_c^l pi = pi s^l
    the identity of a batch          the same under the powers of r: four sums
    the transcript                   the reference's (eip7594.c:390-482) with the cell size a parameter, with hashlib

Also the index maps of csrc/coset_verify_plan.hpp in model form and the stage values the GPU stage tests compare with
(N = 4096 there)."""
import functools
import hashlib

from coset_expect import evaluate, log2
from domain_expect import R, brp, root_of_unity

N_BLOB = 4096


# ---- index maps (csrc/coset_verify_plan.hpp) ----

def cosets(e, N=N_BLOB):
    return (2 * N) >> e


def coset_brp(c, e, N=N_BLOB):
    """the exponent of x_c = w^brp(c), over log2(2N) - e bits"""
    return brp(c, log2(2 * N) - e)


def shift_root(c, e, N=N_BLOB):
    """index into the 2N roots of unity of x_c^l"""
    return (coset_brp(c, e, N) << e) % (2 * N)


def unshift_root(c, e, k, N=N_BLOB):
    """index of x_c^-k"""
    return (2 * N - coset_brp(c, e, N)) * k % (2 * N)


def slot(c, e, j):
    return (c << e) + j


def twiddle_root(pos, s, N=N_BLOB):
    """stage s of the inverse transform of a column: index of w_{2^s}^-(pos mod 2^(s-1))"""
    half = 1 << (s - 1)
    return (2 * N - (pos & (half - 1)) * ((2 * N) >> s)) % (2 * N)


def agg_parts(items, e, per_lane=4, max_parts=16, N=N_BLOB):
    parts = 1
    while parts < max_parts and parts * cosets(e, N) * per_lane < items:
        parts *= 2
    return parts


@functools.lru_cache(maxsize=None)
def roots(N=N_BLOB):
    """w^i for i < 2N"""
    w, out = root_of_unity(2 * N), [1] * (2 * N)
    for i in range(1, 2 * N):
        out[i] = out[i - 1] * w % R
    return out


# ---- the check ----

def x_of(c, e, N=N_BLOB):
    return pow(root_of_unity(2 * N), coset_brp(c, e, N), R)


def interp_coeffs(ys, c, e, N=N_BLOB):
    """the coefficients of the polynomial of degree < l through (x_c w_l^brp_e(j), ys[j])"""
    l = 1 << e
    assert len(ys) == l
    wl_inv = pow(root_of_unity(2 * N), -((2 * N) // l), R)
    xinv, linv = pow(x_of(c, e, N), -1, R), pow(l, -1, R)
    return [pow(xinv, k, R) * linv % R * sum(y * pow(wl_inv, brp(j, e) * k, R) for j, y in enumerate(ys)) % R for k in range(l)]


def column_coeffs(ys, e, N=N_BLOB):
    """stage 4 alone: the inverse transform of one column over the l-th roots of unity, the coset factor left in"""
    l, rt = 1 << e, roots(N)
    linv, step = pow(l, -1, R), (2 * N) // l
    rev = [brp(j, e) for j in range(l)]
    return [linv * sum(y * rt[-rev[j] * k * step % (2 * N)] for j, y in enumerate(ys)) % R for k in range(l)]


def item_holds(commit, c, ys, pi, s, e, N=N_BLOB):
    """C - I(s) + x_c^l pi = pi s^l, with commit = p(s) and pi = q_c(s)"""
    l = 1 << e
    xl = pow(root_of_unity(2 * N), shift_root(c, e, N), R)
    lhs = (commit - evaluate(interp_coeffs(ys, c, e, N), s) + xl * pi) % R
    return lhs == pi * pow(s, l, R) % R


def batch_sums(items, r, s, e, N=N_BLOB):
    """items: (commit, c, ys, pi).  The four sums of the batch: sum r^i pi_i, sum_j w_j C_j over the distinct commitments,
    sum r^i x_c^l pi_i, and the commitment to sum r^i I_i -- the last through the aggregate, as the device makes it."""
    l, w = 1 << e, root_of_unity(2 * N)
    rp = [pow(r, i, R) for i in range(len(items))]
    proof_lc = sum(p * it[3] for p, it in zip(rp, items)) % R
    weights = {}
    for p, it in zip(rp, items):
        weights[it[0]] = (weights.get(it[0], 0) + p) % R
    csum = sum(wt * cm for cm, wt in weights.items()) % R
    wsum = sum(p * pow(w, shift_root(it[1], e, N), R) % R * it[3] for p, it in zip(rp, items)) % R
    interp = interp_sum(aggregate(items, rp, e, N), e, N)
    interp_commit = sum(a * pow(s, k, R) for k, a in enumerate(interp)) % R
    assert len(interp) == l
    return proof_lc, csum, wsum, interp_commit


def batch_holds(items, r, s, e, N=N_BLOB):
    proof_lc, csum, wsum, interp_commit = batch_sums(items, r, s, e, N)
    return (csum - interp_commit + wsum) % R == proof_lc * pow(s, 1 << e, R) % R


# ---- the device's stages ----

def scalars(items, r, e, N=N_BLOB):
    """per item r^i and r^i x_c^l; per distinct commitment (in order of first appearance) its weight"""
    w = root_of_unity(2 * N)
    rp = [pow(r, i, R) for i in range(len(items))]
    wrp = [p * pow(w, shift_root(it[1], e, N), R) % R for p, it in zip(rp, items)]
    order, weights = [], {}
    for p, it in zip(rp, items):
        if it[0] not in weights:
            order.append(it[0])
        weights[it[0]] = (weights.get(it[0], 0) + p) % R
    return rp, wrp, [weights[cm] for cm in order]


def aggregate(items, rp, e, N=N_BLOB):
    """agg[slot(c, j)] = sum over the items of coset c of r^i y_i[j]: always 2N values"""
    agg = [0] * (2 * N)
    for p, it in zip(rp, items):
        for j, y in enumerate(it[2]):
            t = slot(it[1], e, j)
            agg[t] = (agg[t] + p * y) % R
    return agg


def columns_coeffs(agg, e, N=N_BLOB):
    l = 1 << e
    out = []
    for c in range(cosets(e, N)):
        col = agg[c * l:(c + 1) * l]
        out.extend(column_coeffs(col, e, N) if any(col) else col)
    return out


def interp_sum(agg, e, N=N_BLOB):
    """interp[k] = sum_c coeffs[c][k] x_c^-k"""
    return fold(columns_coeffs(agg, e, N), e, 0, cosets(e, N), N)


def fold(coeffs, e, first, last, N=N_BLOB):
    """sum over the columns first .. last - 1 of coeffs[c][k] x_c^-k"""
    l, rt = 1 << e, roots(N)
    out = [0] * l
    for c in range(first, last):
        if any(coeffs[c * l:(c + 1) * l]):
            for k in range(l):
                out[k] = (out[k] + coeffs[c * l + k] * rt[unshift_root(c, e, k, N)]) % R
    return out


# ---- the transcript ----

def transcript(commitments48, coset_indices, evals, proofs48, e, n_blob=N_BLOB):
    """the bytes that are hashed: commitments48[i] names item i's commitment; evals[i] its l * 32 bytes"""
    uniq = []
    for c in commitments48:
        if c not in uniq:
            uniq.append(c)
    out = [b"RCKZGCBATCH__V1_", n_blob.to_bytes(8, "big"), (1 << e).to_bytes(8, "big"), len(uniq).to_bytes(8, "big"),
           len(evals).to_bytes(8, "big")] + uniq
    for cm, c, ev, pf in zip(commitments48, coset_indices, evals, proofs48):
        assert len(ev) == 32 << e and len(pf) == 48 and len(cm) == 48
        out += [uniq.index(cm).to_bytes(8, "big"), c.to_bytes(8, "big"), ev, pf]
    return b"".join(out)


def challenge(commitments48, coset_indices, evals, proofs48, e):
    return int.from_bytes(hashlib.sha256(transcript(commitments48, coset_indices, evals, proofs48, e)).digest(), "big") % R

