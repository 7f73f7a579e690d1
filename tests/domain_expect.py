"""The layout's reference for ckzg_hip_compute_domain_kzg_proofs_batch: the openings of one polynomial at every N-th
root of unity as one Toeplitz product through a circulant of length 2N and one transform (FK20 in its single-point
form), in Python integers with a KNOWN secret s and scalars in place of points ([a]G is written a), against the
definition of the quotient.  Also the integer transforms and blob helpers the GPU tests share."""
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def root_of_unity(n):
    """the n-th root of unity the trusted setup uses (n a power of two up to 2^32): 7^((r - 1) / n)"""
    assert n & (n - 1) == 0 and (R - 1) % n == 0
    return pow(7, (R - 1) // n, R)


def brp(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def fft(vals, w):
    """out[k] = sum_m vals[m] w^(k m) mod r, len(vals) a power of two, w a primitive len(vals)-th root of unity"""
    n = len(vals)
    if n == 1:
        return list(vals)
    w2 = w * w % R
    even, odd = fft(vals[0::2], w2), fft(vals[1::2], w2)
    out, t = [0] * n, 1
    for k in range(n // 2):
        x = t * odd[k] % R
        out[k] = (even[k] + x) % R
        out[k + n // 2] = (even[k] - x) % R
        t = t * w % R
    return out


def ifft_unscaled(vals, w):
    return fft(vals, pow(w, -1, R))


def openings_by_definition(c, s, N):
    """pi(w^k) for k < N from q_x(X) = sum_m x^m sum_{i > m} c_i X^(i - m - 1), evaluated at the secret"""
    w = root_of_unity(N)
    spow = [pow(s, e, R) for e in range(N)]
    inner = [sum(c[i] * spow[i - m - 1] for i in range(m + 1, N)) % R for m in range(N)]
    out = []
    for k in range(N):
        x = pow(w, k, R)
        out.append(sum(pow(x, m, R) * inner[m] for m in range(N)) % R)
    return out


def circulant(c):
    """v of length 2N: v[0] = c[N-1], v[1 .. N+1] = 0, v[N+2+j] = c[1+j] for j = 0 .. N-3"""
    N = len(c)
    v = [0] * (2 * N)
    v[0] = c[N - 1]
    for j in range(N - 2):
        v[N + 2 + j] = c[1 + j]
    return v


def setup_vector(s, N):
    """X of length 2N: X[t] = [s^(N-2-t)] for t <= N-2 (g1_values_monomial reversed from index N-2), the identity above"""
    return [pow(s, N - 2 - t, R) if t <= N - 2 else 0 for t in range(2 * N)]


def openings_by_layout(c, s, N):
    """the steps the device runs: xhat = FFT_2N(X); u = FFT_2N(v) / 2N (.) xhat; h = IFFT_unscaled_2N(u)[:N]; pi = FFT_N(h)"""
    w2 = root_of_unity(2 * N)
    xhat = fft(setup_vector(s, N), w2)
    inv = pow(2 * N, -1, R)
    vhat = [a * inv % R for a in fft(circulant(c), w2)]
    u = [a * b % R for a, b in zip(vhat, xhat)]
    h = ifft_unscaled(u, w2)[:N]
    return h, fft(h, root_of_unity(N))


def h_by_definition(c, s, N):
    """h_m = sum_{i = m+1}^{N-1} c_i [s^(i-m-1)] for m <= N-2, h_{N-1} = the identity"""
    return [sum(c[i] * pow(s, i - m - 1, R) for i in range(m + 1, N)) % R for m in range(N)]


# ---- blobs (N = 4096) ----

def blob_of_poly(c):
    """the blob whose polynomial has the monomial coefficients c (len <= 4096): element j is p(w^brp12(j))"""
    c = list(c) + [0] * (4096 - len(c))
    ev = fft(c, root_of_unity(4096))
    return b"".join(ev[brp(j, 12)].to_bytes(32, "big") for j in range(4096))


def domain_points():
    """z_j = brp_roots_of_unity[j] as 32 big-endian bytes, j < 4096"""
    w = root_of_unity(4096)
    pw = [1] * 4096
    for i in range(1, 4096):
        pw[i] = pw[i - 1] * w % R
    return [pw[brp(j, 12)].to_bytes(32, "big") for j in range(4096)]
