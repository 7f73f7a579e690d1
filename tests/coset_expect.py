"""The layout's reference for ckzg_hip_compute_coset_kzg_proofs_batch: the multiproofs of one polynomial (N coefficients)
on every coset of l = 2^e points of the 2N-point extended domain, in Python integers with a KNOWN secret s and scalars
in place of points ([a]G is written a).  Four things, each by two routes (tests/test_coset_expect_cpu.py):

    the openings by definition      q_c = floor(p / (X^l - x_c^l)) at the secret, by long division
    the openings by the layout      l Toeplitz columns of length 2k (k = N / l), their transforms times the transformed
                                    setup columns, the sum over the columns, an inverse and a forward transform
    the ladder between sizes        pi_e[c] = (pi_{e-1}[2c] - pi_{e-1}[2c+1]) / (2 a), a = x_c^(l/2)
    the order of the cosets         coset c = brp_roots[c l .. c l + l - 1] = x_c times the l-th roots of unity

Also the index maps of csrc/g1_fft_plan.hpp in model form and the helpers the GPU tests share."""
from domain_expect import R, brp, fft, ifft_unscaled, root_of_unity


def log2(n):
    assert n > 0 and n & (n - 1) == 0
    return n.bit_length() - 1


def brp_roots(n):
    """brp_roots_of_unity of the n-point domain: w_n^brp(j)"""
    w, bits = root_of_unity(n), log2(n)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * w % R
    return [pw[brp(j, bits)] for j in range(n)]


def coset_points(N, l, c):
    """the l points of coset c of the 2N-point extended domain, in the order of the evaluations"""
    return brp_roots(2 * N)[c * l:(c + 1) * l]


def evaluate(p, x):
    acc = 0
    for a in reversed(p):
        acc = (acc * x + a) % R
    return acc


# ---- by definition ----

def quotient(p, l, a):
    """floor(p / (X^l - a)): q_i = p[i + l] + a q_{i + l}, from the top"""
    n = len(p)
    q = [0] * max(n - l, 0)
    for i in range(n - l - 1, -1, -1):
        q[i] = (p[i + l] + (a * q[i + l] if i + l < n - l else 0)) % R
    return q


def remainder(p, l, a):
    """p mod (X^l - a): r_j = sum_t p[j + t l] a^t"""
    return [sum(p[j + t * l] * pow(a, t, R) for t in range((len(p) - j + l - 1) // l)) % R for j in range(min(l, len(p)))]


def openings_by_definition(p, s, N, l):
    """pi[c] = q_c(s) for the 2N / l cosets, in the order of the interface"""
    roots = brp_roots(2 * N)
    return [evaluate(quotient(p, l, pow(roots[c * l], l, R)), s) for c in range(2 * N // l)]


# ---- by the layout (src/eip7594/fk20.c at any cell size) ----

def circulant_columns(p, l):
    """toeplitz_coeffs_stride(p, i, l) for i < l: v_i[0] = p[N-1-i], v_i[1 .. k+1] = 0, v_i[k+2+t] = p[2l - i - 1 + t l]"""
    N = len(p)
    k = N // l
    cols = []
    for i in range(l):
        v = [0] * (2 * k)
        v[0] = p[N - 1 - i]
        for t in range(k - 2):
            v[k + 2 + t] = p[2 * l - i - 1 + t * l]
        cols.append(v)
    return cols


def setup_columns(s, N, l):
    """X_i[j] = [s^(N - l - 1 - i - j l)] for j < k - 1, the identity above (setup.c: init_fk20_multi_settings)"""
    k = N // l
    return [[pow(s, N - l - 1 - i - j * l, R) if j < k - 1 else 0 for j in range(2 * k)] for i in range(l)]


def circulant_source(t, e, N):
    """what slot t of the row of 2N (the l columns back to back) reads: a coefficient index or -1"""
    l, k = 1 << e, N >> e
    i, pos = divmod(t, 2 * k)
    if pos == 0:
        return N - 1 - i
    if pos >= k + 2:
        return 2 * l - i - 1 + (pos - k - 2) * l
    return -1


def setup_source(t, e, N):
    l, k = 1 << e, N >> e
    i, j = divmod(t, 2 * k)
    return N - l - 1 - i - j * l if j < k - 1 else -1


def h_by_layout(p, s, N, l):
    """h of length k: the column transforms / 2k times the setup transforms, summed over the columns, inverse transform"""
    k = N // l
    w = root_of_unity(2 * k)
    inv = pow(2 * k, -1, R)
    u = [0] * (2 * k)
    for v, x in zip(circulant_columns(p, l), setup_columns(s, N, l)):
        vhat, xhat = fft(v, w), fft(x, w)
        u = [(acc + a * inv % R * b) % R for acc, a, b in zip(u, vhat, xhat)]
    return ifft_unscaled(u, w)[:k]


def h_by_definition(p, s, N, l):
    """h_j = sum_{i >= (j+1) l} p_i [s^(i - (j+1) l)] for j < k: the proofs are sum_j x^(l j) h_j"""
    k = N // l
    return [sum(p[i] * pow(s, i - (j + 1) * l, R) for i in range((j + 1) * l, N)) % R for j in range(k)]


def openings_by_layout(p, s, N, l):
    k = N // l
    h = h_by_layout(p, s, N, l) + [0] * k
    pi = fft(h, root_of_unity(2 * k))
    bits = log2(2 * k)
    return [pi[brp(c, bits)] for c in range(2 * k)]   # the DIF output order


# ---- the ladder ----

def ladder_step(lower, N, l):
    """the openings at coset size l from those at l / 2"""
    roots = brp_roots(2 * N)
    out = []
    for c in range(2 * N // l):
        a = pow(roots[c * l], l // 2, R)
        out.append((lower[2 * c] - lower[2 * c + 1]) * pow(2 * a, -1, R) % R)
    return out


# ---- blobs (N = 4096) ----

def ext_domain_points():
    """z_j = brp_roots_of_unity[j] of the 8192-point domain as integers"""
    return brp_roots(8192)


def ext_evaluations(c):
    """the 8192 extended evaluations of the polynomial with coefficients c (len <= 4096), in cell order, as integers"""
    c = list(c) + [0] * (8192 - len(c))
    ev = fft(c, root_of_unity(8192))
    return [ev[brp(j, 13)] for j in range(8192)]
