"""What the stages that move and combine vectors of Fr must produce, as Python integers: the transforms of ntt.hip,
evaluation in evaluation form and the opening quotient (verify.hip: k_eval_tree, k_eval_barycentric,
k_quotient_in_domain), the two products of coset_recover_factors.hpp at cosets of 64, and the aggregate and
interpolation sums as the kernels' comments write them.  Nothing here reads the library under test.  Shared by tests/test_gpu_poly_stages.py (the
device stages) and tests/test_poly_expect_cpu.py, which checks each reference by a second route."""
from rlc_expect import R, brev7

N_EXT = 8192
N_BLOB = 4096
VALUE_CLASSES = ("random", "max", "zero", "one_at_0", "one_at_1", "one_at_half", "one_at_last", "ramp")


def brp(i, bits):
    return int("{:0{}b}".format(i, bits)[::-1], 2) if bits else 0


def values(rnd, n):
    """n values with 0, 1 and R - 1 among them (from n = 3 on), the rest random"""
    vals = [rnd.randrange(R) for _ in range(n)]
    if n >= 3:
        vals[n // 2], vals[n - 1], vals[0] = 0, R - 1, 1
    return vals


def class_vector(rnd, cls, n):
    """a vector of n elements of the value class VALUE_CLASSES[cls % 8]"""
    name = VALUE_CLASSES[cls % len(VALUE_CLASSES)]
    if name == "random":
        return [rnd.randrange(R) for _ in range(n)]
    if name == "max":
        return [R - 1] * n
    if name == "zero":
        return [0] * n
    if name == "ramp":
        return list(range(n))
    at = {"one_at_0": 0, "one_at_1": 1, "one_at_half": n // 2, "one_at_last": n - 1}[name]
    v = [0] * n
    v[at % n] = 1
    return v


def batch_inv(xs):
    """1 / x for every x (none zero), one inversion in all"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * xs[i] % R
    return out


def horner(coeffs, x):
    y = 0
    for c in reversed(coeffs):
        y = (y * x + c) % R
    return y


def sparse_eval(terms, x):
    """sum of c x^e over the (c, e) of terms"""
    return sum(c * pow(x, e, R) for c, e in terms) % R


# ---- transforms ----

def dft(x, omega):
    """X[k] = sum_i x[i] omega^(i k), natural order in and out; len(x) a power of two, omega of that order"""
    n = len(x)
    if n == 1:
        return list(x)
    even, odd = dft(x[0::2], omega * omega % R), dft(x[1::2], omega * omega % R)
    out, t, h = [0] * n, 1, n // 2
    for k in range(h):
        o = odd[k] * t % R
        out[k] = (even[k] + o) % R
        out[k + h] = (even[k] - o) % R
        t = t * omega % R
    return out


def ntt_omega(roots, logn, inverse):
    """w^(8192 / n), or its inverse"""
    step = N_EXT >> logn
    return roots[N_EXT - step] if inverse else roots[step]


def ntt(vec, roots, logn, dif, inverse, scale):
    """one transform of fr_ntt_batch.  DIF: out[brp(k)] = sum_i in[i] omega^(ik); DIT: out[k] = sum_i in[brp(i)] omega^(ik);
    times 1 / n when scaling"""
    n = 1 << logn
    assert len(vec) == n
    omega = ntt_omega(roots, logn, inverse)
    if dif:
        X = dft(vec, omega)
        out = [X[brp(k, logn)] for k in range(n)]
    else:
        out = dft([vec[brp(i, logn)] for i in range(n)], omega)
    return times_inv_n(out, logn) if scale else out


def times_inv_n(out, logn):
    ninv = pow(1 << logn, -1, R)
    return [v * ninv % R for v in out]


# ---- evaluation form over the bit-reversed 4096-domain ----

def blob_domain(roots):
    """w_i, i < 4096: the 4096th roots of unity in bit-reversed order (w_1 = -1, w_{2j+1} = -w_{2j})"""
    return [roots[2 * brp(i, 12)] for i in range(N_BLOB)]


def eval_form(poly, z, dom, index=None):
    """p(z) for p given by its values on dom: p_m if z = w_m, else (z^4096 - 1) / 4096 * sum_i p_i w_i / (z - w_i)
    (zero terms are skipped: a blob with one non-zero leaf costs one inversion)"""
    index = index if index is not None else {w: i for i, w in enumerate(dom)}
    if z in index:
        return poly[index[z]]
    at = [i for i in range(N_BLOB) if poly[i]]
    inv = batch_inv([(z - dom[i]) % R for i in at])
    s = sum(poly[i] * dom[i] % R * v for i, v in zip(at, inv)) % R
    return s * (pow(z, N_BLOB, R) - 1) % R * pow(N_BLOB, -1, R) % R


def quotient(poly, z, dom, index=None):
    """(y, hit, q) of the opening of p at z, q in evaluation form.  z off the domain: q_i = (p_i - y) / (w_i - z).
    z = w_m: the same for i != m, and q_m = sum_{i != m} (p_i - y) w_i / (w_m (w_m - w_i))"""
    index = index if index is not None else {w: i for i, w in enumerate(dom)}
    m = index.get(z, -1)
    y = eval_form(poly, z, dom, index)
    others = [i for i in range(N_BLOB) if i != m]
    inv = batch_inv([(dom[i] - z) % R for i in others])
    q = [0] * N_BLOB
    for i, v in zip(others, inv):
        q[i] = (poly[i] - y) * v % R
    if m >= 0:
        # (p_i - y) w_i / (w_m (w_m - w_i)) = -q_i w_i / w_m
        q[m] = -sum(q[i] * dom[i] for i in others) * pow(z, -1, R) % R
    return y, m, q


# ---- recovery: coset_recover_factors.hpp at cosets of 64 ----

SEVEN64 = pow(7, 64, R)


def set_factors(held, roots):
    """(Z over the domain, 1 / Z over the coset) per cell, for the set of held cells: Z vanishes on the missing ones"""
    missing = [j for j in range(128) if j not in held]
    zd, zc = [], []
    for c in range(128):
        xd = roots[64 * brev7(c)]
        xc = SEVEN64 * xd % R
        pd = pc = 1
        for j in missing:
            rj = roots[64 * brev7(j)]
            pd = pd * (xd - rj) % R
            pc = pc * (xc - rj) % R
        zd.append(pd)
        zc.append(pc)
    return zd, batch_inv(zc)


def mask_words(held):
    """bit j of word j / 32 set = cell j is held"""
    w = [0, 0, 0, 0]
    for j in held:
        w[j >> 5] |= 1 << (j & 31)
    return w


# ---- aggregation and interpolation ----

def cell_aggregate(cell_fr, rp, row_start, order):
    """rows[t][j] = sum over the cells i = order[row_start[t] .. row_start[t + 1]) of rp[i] * cell_fr[i][j]"""
    out = []
    for t in range(len(row_start) - 1):
        cells = order[row_start[t]:row_start[t + 1]]
        out.append([sum(rp[i] * cell_fr[i][j] for i in cells) % R for j in range(64)])
    return out


def interp_sum(rows, row_col, roots):
    """interp[k] = sum over the rows t of rows[t][k] * (h_c^-1)^k, c = row_col[t], h_c^-1 = w^(8192 - brp7(c))"""
    return [sum(rows[t][k] * roots[((N_EXT - brev7(c)) * k) % N_EXT] for t, c in enumerate(row_col)) % R for k in range(64)]
