"""Corpora and exact references for the operations of c-kzg-4844_amd/csrc/field_test_ops.hpp: Mont<Fp> / Mont<Fr>
(field.hpp), Fr on 29-bit limbs (fr29.hpp), the safegcd inversions (fp28_inv.hpp, fr_inv.hpp, fr29_inv) and the pairing
tower (tower.hpp, pairing_dev.hpp, against tests/tower_ref.py).  Seeded and deterministic; every comparison is exact
equality of words, or -- where a routine's result is lazily reduced and its representative is the routine's own
business (fr29_inv, f28_inv_safegcd) -- exact congruence plus the bound its header states.
tests/test_field_corpora_cpu.py runs the corpora through the g++ build, tests/test_gpu_fields.py through the device
build.

A corpus is (items, wants): items[i] = the operands (a, b, c, d) of item i as lists of 32-bit words (None: unused),
wants[i] = the expected result words, or a function of the result words that asserts."""
import functools
import random
from fractions import Fraction

import tower_ref as tw

P = tw.P
R = tw.R
SUBSET_LEN = 101          # the first items of every list run again in workgroups of 64: a wave with 37 live lanes
RANDOM_PAIRS = 200
M29 = (1 << 29) - 1
R261 = 1 << 261
TABLE_WORDS = 2 * 68 * 24


def words(v, n):
    assert 0 <= v < 1 << (32 * n), (v, n)
    return [(v >> (32 * j)) & 0xffffffff for j in range(n)]


def value(ws):
    return sum(w << (32 * j) for j, w in enumerate(ws))


def parse_ops(desc):
    """[(name, [wo, wa, wb, wc, wd], shared)] from fieldtest::desc()"""
    ops = []
    for line in desc.strip().split("\n"):
        f = line.split()
        ops.append((f[0], [int(x) for x in f[1:6]], int(f[6])))
    return ops


MONT_KINDS = ["mul", "sqr", "add", "sub", "neg", "dbl", "to_raw", "from_raw", "inv"]
REQUIRED_OPS = (["%s_%s" % (f, k) for f in ("fp", "fr") for k in MONT_KINDS] + ["fr_geq_r"] +
                ["fr29_pack", "fr29_unpack", "fr29_mul", "fr29_mul_inline", "fr29_add", "fr29_carry"] +
                ["fr29_sub_below_%d" % k for k in (0, 2, 3, 5)] + ["fr29_canonical_%d" % k for k in (0, 1, 2, 4, 5)] +
                ["fr29_equal", "fr29_from_fr", "fr29_to_fr", "to_fr_radix256", "vanishing_over_n", "scale", "tree_leaf"] +
                ["tree_combine_%d_%s" % (c, f) for c in range(6) for f in ("call", "flat")] +
                ["tree_canonical_%d" % l for l in range(1, 7)] + ["tree_finish", "tree_finish_from_integers"] +
                ["fr_inv_safegcd", "fr29_inv", "f28_inv_safegcd"] +
                ["fp2_mul", "fp2_sqr", "fp2_inv", "fp2_mul_xi", "fp2_conj", "fp2_mul_fp"] +
                ["fp6_mul", "fp6_inv", "fp6_mul_v", "fp6_mul_sparse01", "fp6_mul_sparse1_fp"] +
                ["fp12_mul", "fp12_sqr", "fp12_inv", "fp12_conj", "fp12_select", "fp12_is_one", "fp12_mul_by_prepared_line"] +
                ["frobenius_1", "frobenius_2", "frobenius_3", "cyclotomic_sqr", "pow_x", "final_exp",
                 "miller_product_tables", "pairing_product_is_one"])
PAIRING_OPS = ("miller_product_tables", "pairing_product_is_one")     # their corpora need the host shim's G2 tables


# ------------------------------------------------------------------------------------------------------------------
# Mont<P>: N words, Montgomery radix 2^(32 N)
# ------------------------------------------------------------------------------------------------------------------
FIELDS = {"fp": (P, 12), "fr": (R, 8)}


def mont_edges(m):
    return [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2]


def mont_specials(m, n):
    """words all 0xffffffff wherever the value stays below m, single-word and single-bit values"""
    out = []
    for k in range(1, n + 1):
        if (1 << (32 * k)) - 1 < m:
            out.append((1 << (32 * k)) - 1)
    top = (m >> (32 * (n - 1))) - 1
    out.append((top << (32 * (n - 1))) | ((1 << (32 * (n - 1))) - 1))       # every lower word all ones, below m
    for k in range(n):
        for w in (1, 0x80000000, 0xffffffff, 0xfffffffe):
            if (w << (32 * k)) < m:
                out.append(w << (32 * k))
    for b in range(m.bit_length()):
        if b % 32 in (0, 1, 15, 30, 31) and (1 << b) < m:
            out.append(1 << b)
    return sorted(set(out))


def cios(a, b, m, n):
    """(t, q): t = (a b + q m) >> 32 n, the value before the final conditional subtraction"""
    rr = 1 << (32 * n)
    q = (-a * b * pow(m, -1, rr)) % rr
    t, rem = divmod(a * b + q * m, rr)
    assert rem == 0
    return t, q


@functools.lru_cache(maxsize=None)
def mont_pairs(field):
    m, n = FIELDS[field]
    rnd = random.Random(7000 + n)
    edges, spec = mont_edges(m), mont_specials(m, n)
    pairs = [(a, b) for a in edges for b in edges]
    pairs += [(s, spec[(i * 7 + 3) % len(spec)]) for i, s in enumerate(spec)]
    pairs += [(s, edges[i % len(edges)]) for i, s in enumerate(spec)] + [(m - 1, s) for s in spec]
    pairs += [(rnd.randrange(m), rnd.randrange(m)) for _ in range(RANDOM_PAIRS)]
    # the first SUBSET_LEN items hold every class: the edge square, then specials and random ones
    subtracted = [pr for pr in pairs[49:] if cios(pr[0], pr[1], m, n)[0] >= m]
    head = pairs[:49] + subtracted[:6] + pairs[49:49 + 20] + pairs[-26:]
    seen = set()
    pairs = [pr for pr in head + pairs if not (pr in seen or seen.add(pr))]
    # both outcomes of the final conditional subtraction occur, in the head too
    for part in (pairs, pairs[:SUBSET_LEN]):
        ts = [cios(a, b, m, n)[0] for a, b in part]
        assert any(t >= m for t in ts) and any(t < m for t in ts), field
        assert all(t < 2 * m for t in ts)
    return pairs


def mont_corpus(field, kind):
    m, n = FIELDS[field]
    rr = 1 << (32 * n)
    rinv = pow(rr, -1, m)
    pairs = mont_pairs(field)
    if kind == "from_raw":       # any n-word integer
        rnd = random.Random(7100 + n)
        xs = [0, 1, m - 1, m, m + 1, 2 * m, 2 * m + 1, rr - 1, rr - 2, rr - m, (rr - 1) // m * m, (rr - 1) // m * m - 1]
        xs += [a for a, _ in pairs[:60]] + [rnd.randrange(rr) for _ in range(RANDOM_PAIRS)]
        return [(words(x, n), None, None, None) for x in xs], [words(x * rr % m, n) for x in xs]
    ref = {"mul": lambda a, b: a * b * rinv % m, "sqr": lambda a, b: a * a * rinv % m, "add": lambda a, b: (a + b) % m,
           "sub": lambda a, b: (a - b) % m, "neg": lambda a, b: -a % m, "dbl": lambda a, b: 2 * a % m,
           "to_raw": lambda a, b: a * rinv % m, "inv": lambda a, b: pow(a, -1, m) * rr * rr % m if a else 0}[kind]
    if kind == "inv":
        pairs = pairs[:49:7] + pairs[49:49 + 30] + pairs[-24:]          # a Fermat ladder each: a short list
    binary = kind in ("mul", "add", "sub")
    if kind == "mul":
        for a, b in pairs:
            t, _ = cios(a, b, m, n)
            assert (t - m if t >= m else t) == ref(a, b)
    items = [(words(a, n), words(b, n) if binary else None, None, None) for a, b in pairs]
    return items, [words(ref(a, b), n) for a, b in pairs]


def geq_corpus():
    rnd = random.Random(7200)
    xs = [R - 1, R, R + 1, 0, (1 << 256) - 1, 1, 2 * R, R - (1 << 255) % R]
    for k in range(8):
        xs += [R + (1 << (32 * k)), R - (1 << (32 * k)), (R ^ (0xffffffff << (32 * k))) & ((1 << 256) - 1)]
    xs += [rnd.randrange(1 << 256) for _ in range(100)]
    return [(words(x, 8), None, None, None) for x in xs], [[1 if x >= R else 0] for x in xs]


# ------------------------------------------------------------------------------------------------------------------
# Fr29: nine 29-bit limbs, Montgomery radix 2^261, lazily reduced
# ------------------------------------------------------------------------------------------------------------------
def limbs29(v):
    """the limbs of v with the top one holding what is left"""
    assert 0 <= v < 1 << (232 + 32), v
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def val29(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


R_LIMBS = limbs29(R)
R_INV261 = pow(R, -1, R261)
ONE29 = R261 % R


def lazy_max(units):
    """every low limb at 2^29 - 1, the top limb as large as the value bound `units` * r allows"""
    bound = int(units * R)
    low = (1 << 232) - 1
    top = (bound - 1 - low) >> 232
    assert top >= 0
    return [M29] * 8 + [top]


def lazy_random(rnd, units):
    top_max = lazy_max(units)[8]
    style = rnd.randrange(4)
    if style == 0:
        return [rnd.randrange(1 << 29) for _ in range(8)] + [rnd.randrange(top_max + 1)]
    if style == 1:
        return [rnd.choice((0, 1, M29, M29 - 1, 1 << 28)) for _ in range(8)] + [rnd.choice((0, 1, top_max, top_max // 2))]
    if style == 2:
        return limbs29(rnd.randrange(R))
    return [M29 if rnd.random() < 0.7 else rnd.randrange(1 << 29) for _ in range(8)] + [top_max]


def mont29(a, b):
    """(limbs of t, q, peak): t = (a b + q r) >> 261 exactly, and the column walk of fr29_mul_inline with an unbounded
    accumulator, which must stay below 2^64 and arrive at the same limbs"""
    va, vb = val29(a), val29(b)
    q = (-va * vb * R_INV261) % R261
    t, rem = divmod(va * vb + q * R, R261)
    assert rem == 0
    acc, peak, qd, out = 0, 0, [], []
    for k in range(9):
        acc += sum(a[i] * b[k - i] for i in range(k + 1)) + sum(qd[i] * R_LIMBS[k - i] for i in range(k))
        qd.append(-acc & M29)
        acc += qd[k]
        peak = max(peak, acc)
        assert acc & M29 == 0
        acc >>= 29
    for k in range(9, 17):
        acc += sum(a[i] * b[k - i] + qd[i] * R_LIMBS[k - i] for i in range(k - 8, 9))
        peak = max(peak, acc)
        out.append(acc & M29)
        acc >>= 29
    out.append(acc)
    assert peak < 1 << 64 and acc < 1 << 32
    assert sum(d << (29 * i) for i, d in enumerate(qd)) == q and out == limbs29(t)
    # the header's bound: a < A r, b < B r  ->  t < (A B r / 2^261 + 1) r
    assert Fraction(t, R) < Fraction(va, R) * Fraction(vb, R) * Fraction(R, R261) + 1
    return out, q, peak


def canonical_boundaries(k_max):
    vals = [0, 1, (1 << (k_max + 1)) * R - 1, (1 << (k_max + 1)) * R - 2]
    for k in range(k_max + 1):
        vals += [(1 << k) * R - 1, (1 << k) * R, (1 << k) * R + 1]
    vals += [3 * R - 1, 3 * R, 3 * R + 1][: 3 if k_max >= 1 else 0]
    return vals


@functools.lru_cache(maxsize=None)
def fr29_mul_cases():
    rnd = random.Random(7300)
    worst, canon = lazy_max(17), [limbs29(v) for v in (0, 1, 2, R - 1, R - 2, (R - 1) // 2, ONE29)]
    cases = [(worst, worst), (worst, limbs29(R - 1)), (limbs29(R - 1), worst), (lazy_max(1), lazy_max(1)),
             (lazy_max(2), lazy_max(17)), ([M29] * 8 + [0], [M29] * 8 + [0])]
    cases += [(a, b) for a in canon for b in canon]
    cases += [(lazy_random(rnd, 17), lazy_random(rnd, 17)) for _ in range(RANDOM_PAIRS)]
    # the widest columns hold 8 + 8 full products (the top limbs are short): the accumulator passes 2^61 of its 2^64
    assert max(mont29(a, b)[2] for a, b in cases[:SUBSET_LEN]) > 1 << 61
    return cases


TREE_BOUNDS = [Fraction(1), Fraction(33, 10), Fraction(77, 10), Fraction(166, 10)]   # children of level c % 4, in r
SUB_K_OF_LEVEL = [0, 2, 3, 5]


def tree_children(rnd, c, count):
    """(e, o, x) for tree_combine<c>: children at and below the bound of their level, x a product of canonical values"""
    bound = TREE_BOUNDS[c % 4]
    edge = [limbs29(int(bound * R) - 1), lazy_max(bound) if c % 4 else limbs29(R - 2), limbs29(0)]
    xs = [limbs29(v) for v in (0, 1, R - 1, ONE29, int(Fraction(1008, 1000) * R))]
    out = [(e, o, x) for e in edge for o in edge for x in xs[2:]]
    while len(out) < count:
        def child():
            if c % 4 == 0:
                return limbs29(rnd.randrange(R))
            return lazy_random(rnd, bound)
        out.append((child(), child(), limbs29(rnd.randrange(int(Fraction(1008, 1000) * R)))))
    return out


def tree_combine_ref(c, e, o, x):
    k = SUB_K_OF_LEVEL[c % 4]
    assert val29(o) < (1 << k) * R
    diff = limbs29(val29(e) + (1 << k) * R - val29(o))
    t, _, _ = mont29(x, diff)
    total = val29(e) + val29(o) + val29(t)
    # the header's bound: a node of level c + 1 is below 2 B_c + 1.4
    assert Fraction(total, R) < 2 * TREE_BOUNDS[c % 4] + Fraction(14, 10)
    if (c + 1) % 4 == 0:
        assert total < 64 * R
        return limbs29(total % R)
    return limbs29(total)


def fr29_corpus(name):
    rnd = random.Random(7400 + sum(map(ord, name)))
    un = lambda ls: [(l, None, None, None) for l in ls]
    if name == "fr29_pack":
        xs = [0, 1, R - 1, R, (1 << 256) - 1, (1 << 232) - 1, 1 << 232, 1 << 255] + [(1 << (29 * i)) - 1 for i in range(1, 9)]
        xs += [1 << (29 * i) for i in range(1, 9)] + [rnd.randrange(1 << 256) for _ in range(120)]
        return un([words(x, 8) for x in xs]), [limbs29(x) for x in xs]
    if name == "fr29_unpack":
        xs = [0, 1, R - 1, R, (1 << 256) - 1, (1 << 232) - 1, 1 << 232] + [(1 << (32 * i)) - 1 for i in range(1, 8)]
        xs += [1 << (32 * i) for i in range(1, 8)] + [rnd.randrange(1 << 256) for _ in range(120)]
        return un([limbs29(x) for x in xs]), [words(x, 8) for x in xs]
    if name in ("fr29_mul", "fr29_mul_inline"):
        cases = fr29_mul_cases()
        return [(a, b, None, None) for a, b in cases], [mont29(a, b)[0] for a, b in cases]
    if name == "fr29_add":
        cases = [(lazy_max(17), lazy_max(17)), (limbs29(R - 1), limbs29(R - 1)), (limbs29(0), limbs29(0)), ([M29] * 8 + [0], limbs29(1))]
        cases += [(lazy_random(rnd, 17), lazy_random(rnd, 17)) for _ in range(120)]
        return [(a, b, None, None) for a, b in cases], [limbs29(val29(a) + val29(b)) for a, b in cases]
    if name == "fr29_carry":      # a limb-wise sum of eight values
        groups = [[lazy_max(8)] * 8, [limbs29(R - 1)] * 8, [limbs29(0)] * 8]
        groups += [[lazy_random(rnd, 8) for _ in range(8)] for _ in range(120)]
        sums = [[sum(v[i] for v in g) for i in range(9)] for g in groups]
        wants = [limbs29(sum(val29(v) for v in g)) for g in groups]
        assert all(w[8] < 1 << 29 for w in wants) and max(max(s) for s in sums) > 1 << 31
        return un(sums), wants
    if name.startswith("fr29_sub_below_"):
        k = int(name.rsplit("_", 1)[1])
        cap = (1 << k) * R
        bs = [limbs29(v) for v in (0, 1, cap - 1, cap - 2, cap // 2, R - 1)]
        mins = [limbs29(0), limbs29(1), limbs29(R - 1), lazy_max(17) if k else limbs29(R - 1), limbs29(int(Fraction(166, 10) * R)) if k else limbs29(R - 2)]
        cases = [(a, b) for a in mins for b in bs]
        for _ in range(120):
            cases.append((lazy_random(rnd, 17) if k else limbs29(rnd.randrange(R)), limbs29(rnd.randrange(cap))))
        wants = [limbs29(val29(a) + cap - val29(b)) for a, b in cases]
        assert all(val29(w) < R261 for w in wants)
        return [(a, b, None, None) for a, b in cases], wants
    if name.startswith("fr29_canonical_") or name == "to_fr_radix256":
        k = 5 if name == "to_fr_radix256" else int(name.rsplit("_", 1)[1])
        xs = canonical_boundaries(k) + [rnd.randrange((2 << k) * R) for _ in range(120)]
        if name == "to_fr_radix256":
            return un([limbs29(x) for x in xs]), [words(x % R, 8) for x in xs]
        return un([limbs29(x) for x in xs]), [limbs29(x % R) for x in xs]
    if name == "fr29_equal":
        base = lazy_random(rnd, 17)
        cases = [(base, base, 1), (limbs29(0), limbs29(0), 1)]
        for i in range(9):
            for bit in (0, 13, 28 if i < 8 else 20):
                other = list(base)
                other[i] ^= 1 << bit
                cases.append((base, other, 0))
        for _ in range(60):
            a = lazy_random(rnd, 17)
            cases += [(a, list(a), 1), (a, lazy_random(rnd, 17), 0)]
        cases = [c for c in cases if (c[0] == c[1]) == bool(c[2])]
        return [(a, b, None, None) for a, b, _ in cases], [[w] for _, _, w in cases]
    if name == "fr29_from_fr":
        xs = mont_edges(R) + mont_specials(R, 8)[:40] + [rnd.randrange(R) for _ in range(120)]
        return un([words(x, 8) for x in xs]), [limbs29(x * 32 % R) for x in xs]
    if name == "fr29_to_fr":
        ls = [limbs29(v) for v in mont_edges(R)] + [lazy_max(17), lazy_max(2)] + [lazy_random(rnd, 17) for _ in range(120)]
        inv32 = pow(32, -1, R)
        return un(ls), [words(val29(l) * inv32 % R, 8) for l in ls]
    if name == "vanishing_over_n":
        zs = [limbs29(v) for v in (0, 1, ONE29, R - 1, R - ONE29)] + [limbs29(rnd.randrange(R)) for _ in range(60)]
        wants = []
        for z in zs:
            zn = z
            for _ in range(12):
                zn = mont29(zn, zn)[0]
            got = mont29(limbs29(val29(zn) + R - ONE29), limbs29(1 << 249))[0]
            true_z = val29(z) * pow(R261, -1, R) % R
            assert val29(got) % R == (pow(true_z, 4096, R) - 1) * pow(4096, -1, R) * R261 % R
            wants.append(got)
        return un(zs), wants
    if name == "scale":
        sums = [rnd.randrange(R) for _ in range(100)] + [0, 1, R - 1]
        fs = [lazy_random(rnd, 2) for _ in sums]
        wants = [words(val29(mont29(limbs29(s), f)[0]) % R, 8) for s, f in zip(sums, fs)]
        return [(words(s, 8), f, None, None) for s, f in zip(sums, fs)], wants
    if name == "tree_leaf":
        xs, _ = geq_corpus()
        xs = [value(x[0]) for x in xs]
        return un([words(x, 8) for x in xs]), [(limbs29(x) if x < R else [0] * 9) + [1 if x >= R else 0] for x in xs]
    if name.startswith("tree_combine_"):
        c = int(name.split("_")[2])
        cases = tree_children(random.Random(7500 + c), c, 110)      # the call and flat forms share their corpus
        return [(e, o, x, None) for e, o, x in cases], [tree_combine_ref(c, e, o, x) for e, o, x in cases]
    if name.startswith("tree_canonical_"):
        lvl = int(name.rsplit("_", 1)[1])
        k = {0: None, 1: 1, 2: 2, 3: 4}[lvl % 4]
        if k is None:
            ls = [lazy_random(rnd, 17) for _ in range(110)]
            return un(ls), ls
        bound = int(TREE_BOUNDS[lvl % 4] * R)
        xs = [x for x in canonical_boundaries(k) if x < bound] + [bound - 1] + [rnd.randrange(bound) for _ in range(110)]
        return un([limbs29(x) for x in xs]), [limbs29(x % R) for x in xs]
    if name in ("tree_finish", "tree_finish_from_integers"):
        xs = mont_edges(R) + [rnd.randrange(R) for _ in range(110)]
        factor = pow(4096, -1, R) * ((1 << 256) if name.endswith("integers") else 1)
        return un([limbs29(x) for x in xs]), [words(x * factor % R, 8) for x in xs]
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------
# the safegcd inversions: the inputs are chosen as the integer g that reaches the divsteps
# ------------------------------------------------------------------------------------------------------------------
def divstep_batches(m, x):
    """how many batches of 30 divsteps (fp28_inv.hpp) the pair (m, x) takes until g reaches zero"""
    delta, f, g, n = 1, m, x, 0
    while g:
        if g & 1:
            if delta > 0:
                delta, f, g = 1 - delta, g, (g - f) >> 1
            else:
                delta, g = 1 + delta, (g + f) >> 1
        else:
            delta, g = 1 + delta, g >> 1
        n += 1
    return (n + 29) // 30


def inversion_inputs(m, seed):
    """1, 2, m - 1, (m +- 1)/2, 2^k and 2^k +- 1 across the width, values with 30 to 90 trailing zero bits and random
    ones, dealt out by the number of batches each takes so that the lanes of every wave of 64 leave the loop at
    different times.  (f starts at the full-width modulus, so no input finishes after only a few batches: the counts
    span 17..19 for r and 26..28 for p, and every wave holds the shortest and the longest runs of the list.)"""
    rnd = random.Random(seed)
    bits = m.bit_length()
    vals = [1, 2, 3, 4, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2]
    for k in list(range(5, bits - 1, 11)) + [bits - 2]:
        vals += [1 << k, (1 << k) - 1, (1 << k) + 1]
    for z in range(30, 91, 6):
        vals += [(rnd.randrange(1, 1 << (bits - 2 - z)) | 1) << z, 1 << z]
    vals = sorted({v for v in vals if 0 < v < m})
    waves = (len(vals) + RANDOM_PAIRS + 63) // 64
    vals += [rnd.randrange(1, m) for _ in range(64 * waves - 27 - len(vals))]     # the last wave holds 37
    vals.sort(key=lambda v: (divstep_batches(m, v), v))
    deal = [[] for _ in range(waves)]
    rest, w, back = list(vals), 0, False
    while rest:                                   # the shortest and the longest runs left, wave after wave
        while len(deal[w]) >= (64 if w < waves - 1 else 37):
            w = (w + 1) % waves
        deal[w].append(rest.pop(-1 if back else 0))
        if back:
            w = (w + 1) % waves
        back = not back
    lo, hi = divstep_batches(m, vals[0]), divstep_batches(m, vals[-1])
    assert hi - lo >= 2 and hi <= (26 if bits < 256 else 40)      # the loops' own limits: 26 and 40 batches
    out = []
    for d in deal:
        b = [divstep_batches(m, v) for v in d]
        assert min(b) == lo and max(b) == hi, (min(b), max(b), lo, hi)
        rnd.shuffle(d)
        out += d
    return out


def inversion_corpus(name):
    if name == "fr_inv_safegcd":      # x 2^256 -> (1/x) 2^256, canonical; 0 -> 0
        gs = inversion_inputs(R, 7601) + [0]
        return [(words(g, 8), None, None, None) for g in gs], [words(pow(g, -1, R) * (1 << 512) % R if g else 0, 8) for g in gs]
    if name == "fr29_inv":            # x 2^261 (canonical, != 0) -> 2^261 / x, below 2 r
        gs = inversion_inputs(R, 7602)

        def check(g):
            def f(out):
                assert all(l < 1 << 29 for l in out), out
                assert val29(out) < 2 * R and val29(out) % R == pow(g, -1, R) * (1 << 522) % R, (g, out)
            return f
        return [(limbs29(g), None, None, None) for g in gs], [check(g) for g in gs]
    if name == "f28_inv_safegcd":     # 14 limbs of 28 bits, value below 2 p, radix 2^392; 0 for 0 mod p
        gs = inversion_inputs(P, 7603)
        gs += [0, P] + [g + P for g in gs[:26]]
        l28 = lambda v: [(v >> (28 * j)) & ((1 << 28) - 1) for j in range(14)]

        def check(g):
            def f(out):
                v = sum(l << (28 * j) for j, l in enumerate(out))
                assert all(l < 1 << 28 for l in out), out
                if g % P == 0:
                    assert v == 0, out
                else:
                    assert v < 2 * P and v % P == pow(g, -1, P) * (1 << 784) % P, (g, out)
            return f
        return [(l28(g), None, None, None) for g in gs], [check(g) for g in gs]
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------
# the pairing tower against tower_ref.py
# ------------------------------------------------------------------------------------------------------------------
TOWER_ITEMS = 40
HEAVY_ITEMS = 5


def _rand_el(rnd, deg):
    vals = [rnd.choice((0, 1, P - 1, 2, (P - 1) // 2)) if rnd.random() < 0.15 else rnd.randrange(P) for _ in range(deg)]
    return tw._nest(vals, tw.SHAPES[deg])


def _els(seed, deg, count):
    rnd = random.Random(seed)
    one = tw._nest([1] + [0] * (deg - 1), tw.SHAPES[deg])
    most = tw._nest([P - 1] * deg, tw.SHAPES[deg])
    return [one, most] + [_rand_el(rnd, deg) for _ in range(count - 2)]


@functools.lru_cache(maxsize=None)
def cyclotomic_inputs():
    return [tw.f12_easy_part(f) for f in _els(7700, 12, HEAVY_ITEMS + 1)[1:]]


def _is_one_back(mul, deg, a):
    one = tw.to_words(tw._nest([1] + [0] * (deg - 1), tw.SHAPES[deg]))

    def f(out):
        assert all(value(out[i:i + 12]) < P for i in range(0, len(out), 12)), "not fully reduced"
        assert tw.to_words(mul(a, tw.from_words(out))) == one, "a * inv(a) != 1"
    return f


@functools.lru_cache(maxsize=None)
def tower_corpus(name):
    W = tw.to_words
    seed = 7800 + sum(map(ord, name))
    rnd = random.Random(seed)
    f2, f6, f12 = (lambda n=TOWER_ITEMS, s=0: _els(seed + s, 2, n)), (lambda n=TOWER_ITEMS, s=0: _els(seed + s, 6, n)), \
        (lambda n=TOWER_ITEMS, s=0: _els(seed + s, 12, n))
    un = lambda xs, ref: ([(W(x), None, None, None) for x in xs], [W(ref(x)) for x in xs])
    bi = lambda xs, ys, ref: ([(W(x), W(y), None, None) for x, y in zip(xs, ys)], [W(ref(x, y)) for x, y in zip(xs, ys)])
    f2l = lambda a: (a, tw.F2_ZERO, tw.F2_ZERO)
    if name == "fp2_mul":
        return bi(f2(), f2(s=1), tw.f2_mul)
    if name == "fp2_sqr":
        return un(f2(), lambda a: tw.f2_mul(a, a))
    if name == "fp2_mul_xi":
        return un(f2(), lambda a: tw.f2_mul(a, tw.XI))
    if name == "fp2_conj":
        return un(f2(), tw.f2_conj)
    if name == "fp2_mul_fp":
        xs, ks = f2(), [1, P - 1, 0] + [rnd.randrange(P) for _ in range(TOWER_ITEMS - 3)]
        return [(W(x), W(k), None, None) for x, k in zip(xs, ks)], [W(tw.f2_scale(x, k)) for x, k in zip(xs, ks)]
    if name == "fp6_mul":
        return bi(f6(), f6(s=1), tw.f6_mul)
    if name == "fp6_mul_v":
        return un(f6(), lambda a: tw.f6_mul(a, tw.V6))
    if name == "fp6_mul_sparse01":
        xs, b0, b1 = f6(), f2(s=1), f2(s=2)
        return [(W(x), W(p), W(q), None) for x, p, q in zip(xs, b0, b1)], \
            [W(tw.f6_mul(x, (p, q, tw.F2_ZERO))) for x, p, q in zip(xs, b0, b1)]
    if name == "fp6_mul_sparse1_fp":
        xs, ks = f6(), [1, P - 1, 0] + [rnd.randrange(P) for _ in range(TOWER_ITEMS - 3)]
        return [(W(x), W(k), None, None) for x, k in zip(xs, ks)], \
            [W(tw.f6_mul(x, (tw.F2_ZERO, (k, 0), tw.F2_ZERO))) for x, k in zip(xs, ks)]
    if name == "fp12_mul":
        return bi(f12(), f12(s=1), tw.f12_mul)
    if name == "fp12_sqr":
        return un(f12(), lambda a: tw.f12_mul(a, a))
    if name == "fp12_conj":
        return un(f12(), tw.f12_conj)
    if name in ("fp2_inv", "fp6_inv", "fp12_inv"):      # checked by multiplying back
        deg, mul = {"fp2_inv": (2, tw.f2_mul), "fp6_inv": (6, tw.f6_mul), "fp12_inv": (12, tw.f12_mul)}[name]
        xs = [x for x in _els(seed, deg, TOWER_ITEMS if deg < 12 else 12) if any(tw.flatten(x))]
        if deg == 2:
            xs = [x for x in xs if (x[0] * x[0] + x[1] * x[1]) % P]
        return [(W(x), None, None, None) for x in xs], [_is_one_back(mul, deg, x) for x in xs]
    if name == "fp12_select":                            # both masks
        xs, ys = f12(), f12(s=1)
        items = [(W(x), W(y), [0xffffffff if i % 2 == 0 else 0], None) for i, (x, y) in enumerate(zip(xs, ys))]
        return items, [W(x if i % 2 == 0 else y) for i, (x, y) in enumerate(zip(xs, ys))]
    if name == "fp12_is_one":         # the identity, the identity with one bit flipped in each of the 144 words, a random element
        one = W(tw.F12_ONE)
        items, wants = [(one, None, None, None)], [[1]]
        for i in range(144):
            w = list(one)
            w[i] ^= 1 << ((7 * i + 3) % 32)
            items.append((w, None, None, None))
            wants.append([0])
        items.append((W(_rand_el(rnd, 12)), None, None, None))
        wants.append([0])
        order = list(range(0, 146, 2)) + list(range(1, 146, 2))     # the first SUBSET_LEN items reach words of every coefficient
        return [items[i] for i in order], [wants[i] for i in order]
    if name == "fp12_mul_by_prepared_line":
        fs, lams, cs = f12(), f2(s=1), f2(s=2)
        pts = [(rnd.randrange(P), rnd.randrange(P)) for _ in fs]
        return [(W(f), W(l), W(c), W(p[0]) + W(p[1])) for f, l, c, p in zip(fs, lams, cs, pts)], \
            [W(tw.f12_mul(f, tw.f12_from_line(l, c, p[0], p[1]))) for f, l, c, p in zip(fs, lams, cs, pts)]
    if name.startswith("frobenius_"):
        k = int(name[-1])
        return un(f12(HEAVY_ITEMS), lambda a: tw.f12_frobenius(a, k))
    if name == "cyclotomic_sqr":
        return un(cyclotomic_inputs(), lambda g: tw.f12_mul(g, g))
    if name == "pow_x":
        return un(cyclotomic_inputs(), lambda g: tw.f12_conj(tw.f12_pow(g, tw.X_ABS)))
    if name == "final_exp":
        return un(f12(HEAVY_ITEMS)[1:] + [_rand_el(rnd, 12)], tw.f12_final_exp)
    raise KeyError(name)


def corpus(name):
    """(items, wants) of every operation but the two that take line tables"""
    parts = name.split("_", 1)
    if parts[0] in FIELDS and parts[1] in MONT_KINDS:
        return mont_corpus(parts[0], parts[1])
    if name == "fr_geq_r":
        return geq_corpus()
    if name in ("fr_inv_safegcd", "fr29_inv", "f28_inv_safegcd"):
        return inversion_corpus(name)
    if name.startswith(("fp2_", "fp6_", "fp12_", "frobenius_")) or name in ("cyclotomic_sqr", "pow_x", "final_exp"):
        return tower_corpus(name)
    return fr29_corpus(name)


_CORPUS = {}


def cached_corpus(name):
    if name not in _CORPUS:
        _CORPUS[name] = corpus(name)
    return _CORPUS[name]


def pack(items, widths, shared=False):
    """the four operand buffers of a call as flat word lists; an unused operand is one zero word"""
    bufs = []
    for k in range(4):
        w = widths[1 + k]
        if w == 0:
            assert all(it[k] is None for it in items), k
            bufs.append([0])
            continue
        rows = items[:1] if shared and k >= 2 else items
        flat = []
        for it in rows:
            assert len(it[k]) == w, (k, len(it[k]), w)
            flat += it[k]
        bufs.append(flat)
    return bufs


def check(name, wants, out, wo, count=None):
    count = len(wants) if count is None else count
    for i in range(count):
        got = list(out[wo * i:wo * (i + 1)])
        if callable(wants[i]):
            wants[i](got)
        else:
            assert got == wants[i], (name, i, [hex(x) for x in got], [hex(x) for x in wants[i]])


# ------------------------------------------------------------------------------------------------------------------
# the two-pair Miller product and verdict against line tables of the host shim's prepared G2 points
# ------------------------------------------------------------------------------------------------------------------
INF_AFFINE = [0] * 24


class PairingInputs:
    """G1 / G2 multiples and line tables through libhost_shim.so (ctypes handle h)"""

    def __init__(self, h):
        import ctypes as C
        self.C, self.h = C, h

    def _mul(self, gen, fn, size, k):
        C = self.C
        g, out = C.create_string_buffer(size), C.create_string_buffer(size)
        gen(g)
        fn(out, g, (C.c_uint32 * 8)(*words(k % R, 8)), 255)
        return out.raw

    def g1(self, k):
        return self._mul(self.h.hs_g1_generator, self.h.hs_g1_mul, 144, k)

    def g2(self, k):
        return self._mul(self.h.hs_g2_generator, self.h.hs_g2_mul, 288, k)

    def affine(self, jac):
        if jac[96:] == bytes(48):
            return list(INF_AFFINE)
        out = self.C.create_string_buffer(96)
        self.h.hs_g1_xyzz_to_affine(out, jac)
        return [int.from_bytes(out.raw[4 * j:4 * j + 4], "little") for j in range(24)]

    def table(self, q):
        out = (self.C.c_uint32 * TABLE_WORDS)()
        self.h.hs_g2_line_table(out, q)
        return list(out)

    def host_miller(self, x1, q1, x2, q2):
        out = self.C.create_string_buffer(576)
        self.h.hs_host_miller(out, x1, q1, x2, q2)
        return [int.from_bytes(out.raw[4 * j:4 * j + 4], "little") for j in range(144)]


_FINAL_EXP = {}


def final_exp_ref(ws):
    key = tuple(ws)
    if key not in _FINAL_EXP:
        _FINAL_EXP[key] = tw.f12_final_exp(tw.from_words(list(ws)))
    return _FINAL_EXP[key]


_PAIRING = {}


def pairing_corpus(name, h):
    """One call = one pair of tables ([b]G2, G2).  miller_product_tables: item 0 is e(G1, G2) through the second slot,
    the others e([a]G1, [b]G2) through the first, one with both slots finite; wants = the value of host_pairing.hpp's
    branching Miller product in libhost_shim.so byte for byte, and check_miller_relation ties them together by the
    Python tower alone.  pairing_product_is_one: the case list of test_two_pair_verdicts_match_host, 37 items, infinite
    and finite arguments mixed in both slots."""
    if name in _PAIRING:
        return _PAIRING[name]
    pi = PairingInputs(h)
    rnd = random.Random(14)
    INF1 = bytes(144)
    b = rnd.randrange(1, R)
    q1, g2 = pi.g2(b), pi.g2(1)
    t1, t2 = pi.table(q1), pi.table(g2)
    if name == "miller_product_tables":
        scal = [rnd.randrange(1, R) for _ in range(HEAVY_ITEMS - 2)]
        pts = [(INF1, pi.g1(1))] + [(pi.g1(a), INF1) for a in scal] + [(pi.g1(scal[0]), pi.g1(R - scal[0] * b % R))]
        items = [(pi.affine(x1), pi.affine(x2), t1, t2) for x1, x2 in pts]
        wants = [pi.host_miller(x1, q1, x2, g2) for x1, x2 in pts]
        _PAIRING[name] = (items, wants, (scal, b))
        return _PAIRING[name]
    cases = []
    for rep in range(5):
        a = rnd.randrange(1, R)
        p1, good, bad = pi.g1(a), pi.g1(R - a * b % R), pi.g1(R - a * b % R + 1)
        cases += [(p1, good, 1), (p1, bad, 0), (good, p1, 0), (INF1, INF1, 1), (INF1, good, 0), (p1, INF1, 0), (INF1, pi.g1(0), 1)]
    cases += [(bad, p1, 0), (INF1, p1, 0)]
    assert len(cases) == 37
    for x1, x2, want in cases:
        assert (h.hs_pairing_prepared(x1, q1, x2, g2) & 1) == want
    items = [(pi.affine(x1), pi.affine(x2), t1, t2) for x1, x2, _ in cases]
    assert any(it[0] == INF_AFFINE and it[1] != INF_AFFINE for it in items) and any(it[1] == INF_AFFINE and it[0] != INF_AFFINE for it in items)
    _PAIRING[name] = (items, [[w] for _, _, w in cases], None)
    return _PAIRING[name]


def check_miller_relation(outs, extra):
    """independently of the project's pairing code: final_exp(miller([a]P, [b]Q)) == final_exp(miller(P, Q))^(a b), and the
    pair e([a]P, [b]Q) e([-a b]P, Q) ends at one -- final_exp and the powers by tower_ref.py"""
    scal, b = extra
    base = final_exp_ref(outs[0])
    assert base != tw.F12_ONE
    assert tw.f12_pow(base, R) == tw.F12_ONE
    for a, ws in zip(scal, outs[1:1 + len(scal)]):
        assert final_exp_ref(ws) == tw.f12_pow(base, a * b % R), a
    assert final_exp_ref(outs[1 + len(scal)]) == tw.F12_ONE
