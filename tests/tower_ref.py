"""The BLS12-381 pairing tower on Python integers, written from its definitions:
    Fp2 = Fp[u]/(u^2 + 1),  Fp6 = Fp2[v]/(v^3 - (1 + u)),  Fp12 = Fp6[w]/(w^2 - v)
Schoolbook products, no Karatsuba, no sparse forms, no Frobenius constants, no cyclotomic shortcut: a power is square
and multiply, the Frobenius map is f -> f^(p^K) computed as that power, the final exponentiation is the power
3 (p^12 - 1)/r.  It is the independent reference for c-kzg-4844_amd/csrc/tower.hpp (tests/test_field_corpora_cpu.py,
tests/test_gpu_fields.py); nothing here is taken from it.

An Fp2 is a pair of integers below p, an Fp6 a triple of Fp2, an Fp12 a pair of Fp6.  On the wire an Fp is twelve
32-bit words of x 2^384 mod p, least significant first, and a tower element its coefficients in order."""
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
X_ABS = 0xd201000000010000
MONT = 1 << 384
MONT_INV = pow(MONT, -1, P)
FINAL_EXPONENT = 3 * ((P ** 12 - 1) // R)
assert (P ** 12 - 1) % R == 0

F2_ZERO, F2_ONE, XI = (0, 0), (1, 0), (1, 1)
F6_ZERO, F6_ONE = (F2_ZERO,) * 3, (F2_ONE, F2_ZERO, F2_ZERO)
F12_ONE = (F6_ONE, F6_ZERO)


# ---- Fp2 ----
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):          # (a0 + a1 u)(b0 + b1 u), u^2 = -1
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


# ---- Fp6 ----
def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_neg(a):
    return tuple(f2_neg(x) for x in a)


def f6_mul(a, b):          # sum a_i b_j v^(i + j), v^3 = xi
    c = [F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            c[i + j] = f2_add(c[i + j], f2_mul(a[i], b[j]))
    return (f2_add(c[0], f2_mul(XI, c[3])), f2_add(c[1], f2_mul(XI, c[4])), c[2])


V6 = (F2_ZERO, F2_ONE, F2_ZERO)


# ---- Fp12 ----
def f12_mul(a, b):         # (a0 + a1 w)(b0 + b1 w), w^2 = v
    return (f6_add(f6_mul(a[0], b[0]), f6_mul(V6, f6_mul(a[1], b[1]))), f6_add(f6_mul(a[0], b[1]), f6_mul(a[1], b[0])))


def f12_conj(a):
    return (a[0], f6_neg(a[1]))


def f12_pow(a, e):
    acc = F12_ONE
    for bit in bin(e)[2:]:
        acc = f12_mul(acc, acc)
        if bit == "1":
            acc = f12_mul(acc, a)
    return acc


def f12_frobenius(a, k):
    return f12_pow(a, P ** k)


def f12_final_exp(a):
    return f12_pow(a, FINAL_EXPONENT)


def f12_easy_part(a):
    """a^((p^6 - 1)(p^2 + 1)): an element of the cyclotomic subgroup"""
    return f12_pow(a, (P ** 6 - 1) * (P ** 2 + 1))


def f12_from_line(lam, c, xp, yp):
    """the line value c + (-lam xp) v + yp v w of mul_by_prepared_line"""
    return ((c, f2_neg(f2_scale(lam, xp)), F2_ZERO), (F2_ZERO, (yp, 0), F2_ZERO))


# ---- the wire format ----
def flatten(x):
    if isinstance(x, int):
        return [x]
    return [v for part in x for v in flatten(part)]


def to_words(x):
    out = []
    for v in flatten(x):
        m = v * MONT % P
        out += [(m >> (32 * j)) & 0xffffffff for j in range(12)]
    return out


def _nest(vals, shape):
    if not shape:
        return vals.pop(0)
    return tuple(_nest(vals, shape[1:]) for _ in range(shape[0]))


SHAPES = {1: (), 2: (2,), 6: (3, 2), 12: (2, 3, 2)}


def from_words(words):
    """the element of 12 * k words; the limbs are reduced mod p (a reference value never holds more)"""
    assert len(words) % 12 == 0
    vals = []
    for i in range(0, len(words), 12):
        m = sum(w << (32 * j) for j, w in enumerate(words[i:i + 12]))
        vals.append(m * MONT_INV % P)
    return _nest(vals, SHAPES[len(vals)])
