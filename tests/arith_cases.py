"""Case corpora and exact references shared by the host and the device arithmetic tests
(test_host_arith.py, test_f28_corpora_cpu.py, test_gpu_dev_arith.py).  Everything here is seeded and
deterministic, and nothing here touches a library: the references are Python integers.

Field part.  An F28<L, V> operand is 14 limbs l_j with every limb < L * 2^28 and the value
sum l_j 2^(28 j) <= V * p.  The Montgomery routines must return EXACTLY
    t = (a b [+ c d] + q p) >> 392,   q = -(a b [+ c d]) / p mod 2^392,
as 13 digits of 28 bits and the rest in limb 13; mont_exact() computes that, and replay_columns() walks the 28
columns the way fp28.hpp does with one unbounded accumulator, so that the test can assert the header's claim that
it stays below 2^64 on the very inputs it runs."""
import random

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
LAMBDA = 0xd201000000010000 ** 2 - 1
M28 = (1 << 28) - 1
R392 = 1 << 392
P_INV392 = pow(P, -1, R392)
P_LIMBS = [(P >> (28 * j)) & M28 for j in range(14)]
NINV28 = (-pow(P, -1, 1 << 28)) % (1 << 28)

# the canonical edges of test_host_arith.py's field tests, and values whose top 28-bit limb equals p's (or is one
# below it with the limbs under it high): the family of test_fp28_conditional_negation_top_limb_edge
FP_EDGES = [0, 1, P - 1, P - 2, (P - 1) // 2, 2 ** 380, P - 3]


def top_limb_family(rnd, n):
    out = []
    for k in range(n):
        out.append(((P >> 364 << 364) - rnd.randrange(1 << 300) - 1) if k % 2 else (P - 1 - rnd.randrange(1 << 360)))
    return out


def value(limbs):
    return sum(int(l) << (28 * j) for j, l in enumerate(limbs))


def canonical_limbs(v):
    """13 digits of 28 bits and the rest"""
    assert 0 <= v < 1 << (364 + 32)
    return [(v >> (28 * j)) & M28 for j in range(13)] + [v >> 364]


def _max_top(low, L, V):
    """largest top limb that keeps low + top 2^364 <= V p (None if the low limbs alone exceed it)"""
    rest = V * P - low
    if rest < 0:
        return None
    return min(rest >> 364, L * (1 << 28) - 1)


def operand_worst(L, V):
    if V == 0:
        return [0] * 14
    low = [L * (1 << 28) - 1] * 13
    top = _max_top(value(low), L, V)
    assert top is not None
    return low + [top]


def operand_mix(rnd, L, V):
    if V == 0:
        return [0] * 14
    choices = [c for c in (0, 1, M28, 1 << 28, L * (1 << 28) - 1) if c < L * (1 << 28)]
    while True:
        low = [rnd.choice(choices) for _ in range(13)]
        top = _max_top(value(low), L, V)
        if top is not None:
            return low + [rnd.choice([0, 1, top, top // 2, rnd.randrange(top + 1)])]


def operand_random(rnd, L, V):
    if V == 0:
        return [0] * 14
    while True:
        low = [rnd.randrange(L * (1 << 28)) for _ in range(13)]
        top = _max_top(value(low), L, V)
        if top is not None:
            return low + [rnd.randrange(top + 1)]


def operand_edges(rnd, L, V):
    if V == 0:
        return [[0] * 14]
    vals = FP_EDGES + top_limb_family(rnd, 6)
    if V >= 2:
        vals += [P, P + 1, V * P, V * P - 1]
    return [canonical_limbs(v) for v in vals]


# ---- exact references ----

def mont_exact(pairs):
    """(sum of products + q p) >> 392 and q"""
    x = sum(value(a) * value(b) for a, b in pairs)
    q = (-x * P_INV392) % R392
    t = x + q * P
    assert t % R392 == 0
    return t >> 392, q


def replay_columns(pairs, square=False):
    """fp28.hpp's column walk with an unbounded accumulator: (result limbs, largest accumulator seen).  For
    square=True `pairs` is [(a, a)] and the cross terms are taken once against the doubled operand."""
    q = [0] * 14
    acc = 0
    peak = 0
    out = [0] * 14

    def products(k, lo, hi):
        s = 0
        for a, b in pairs:
            if square:
                for i in range(lo, hi):
                    if 2 * i < k:
                        d = (a[k - i] << 1) & 0xffffffff
                        s += a[i] * d
                if k % 2 == 0:
                    s += a[k // 2] * a[k // 2]
            else:
                for i in range(lo, hi):
                    s += a[i] * b[k - i]
        return s

    for k in range(14):
        acc += products(k, 0, k + 1)
        acc += sum(q[i] * P_LIMBS[k - i] for i in range(k))
        q[k] = (((acc & 0xffffffff) * NINV28) & 0xffffffff) & M28
        acc += q[k] * P_LIMBS[0]
        peak = max(peak, acc)
        acc >>= 28
    for k in range(14, 27):
        acc += products(k, k - 13, 14)
        acc += sum(q[i] * P_LIMBS[k - i] for i in range(k - 13, 14))
        peak = max(peak, acc)
        out[k - 14] = acc & M28
        acc >>= 28
    out[13] = acc
    return out, peak


def parse_ops(desc):
    """the shims' operation list -> [(name, (template arguments...))]"""
    ops = []
    for line in desc.strip().split("\n"):
        f = line.split()
        ops.append((f[0], tuple(int(x) for x in f[1:])))
    return ops


def op_bounds(op):
    """(L, V) of each F28 operand of an operation"""
    name, a = op
    if name in ("mul", "add", "sub", "equal"):
        return [(a[0], a[1]), (a[2], a[3])]
    if name == "sub_k":
        return [(a[1], a[2]), (a[3], a[4])]
    if name == "mul_add2":
        return [(a[2 * i], a[2 * i + 1]) for i in range(4)]
    if name in ("sqr", "norm", "to_fp"):
        return [(a[0], a[1])]
    if name == "is_zero":
        return [(1, 2)]
    if name == "cneg":
        return [(1, 1)]
    if name == "from_fp":
        return []
    raise ValueError(name)


# what the issue requires to be among the instantiations, whatever else the list holds
REQUIRED_OPS = [("mul", (4, 64, 4, 6)), ("mul", (4, 6, 4, 18)), ("mul", (3, 34, 3, 34)), ("mul", (2, 34, 2, 34)),
                ("sqr", (4, 6)), ("sqr", (4, 41)), ("mul_add2", (2, 8, 4, 18, 1, 6, 1, 2)),
                ("mul_add2", (1, 6, 4, 18, 4, 4, 1, 2)), ("mul", (1, 2, 1, 2)), ("sqr", (1, 2)),
                ("mul_add2", (1, 2, 1, 2, 1, 2, 1, 2))]
REQUIRED_KINDS = {"mul", "sqr", "mul_add2", "add", "sub", "sub_k", "norm", "cneg", "from_fp", "to_fp", "is_zero", "equal"}

RANDOM_FILL = 200
QUOTIENT_DRAW_CAP = 400000


def _quotient_cases(rnd, op):
    """operands whose quotient q takes chosen values: all digits 0, all digits 2^28 - 1, one digit 2^28 - 1"""
    name, _ = op
    b = op_bounds(op)
    out = []
    # q = 0: a b [+ c d] divisible by 2^392, from operands that are multiples of 2^196
    def mult196(L, V):
        return canonical_limbs((rnd.randrange(min(V * P, R392 - 1) >> 196) | 1) << 196)
    out.append([mult196(*bd) for bd in b])
    if name == "sqr":
        return out   # a square root modulo 2^392 cannot be chosen freely: the other targets are for the products
    targets = [R392 - 1] + [M28 << (28 * j) for j in (0, 6, 13)]
    (LA, VA), (LB, VB) = b[0], b[1]
    for q in targets:
        for _ in range(QUOTIENT_DRAW_CAP):
            a = operand_random(rnd, LA, VA)
            a[0] |= 1
            if value(a) > VA * P:
                continue
            rest = [operand_random(rnd, *bd) for bd in b[2:]]
            cd = value(rest[0]) * value(rest[1]) if rest else 0
            bv = ((-q * P - cd) * pow(value(a), -1, R392)) % R392
            if bv <= VB * P:
                out.append([a, canonical_limbs(bv)] + rest)
                break
        else:
            raise AssertionError("no operand found for quotient %x of %r" % (q, op))
        got = mont_exact([(out[-1][0], out[-1][1])] + ([(rest[0], rest[1])] if rest else []))[1]
        assert got == q
    return out


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        key = repr(c)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def field_cases(op, seed=2028):
    """every input class for one operation: a list of operand tuples (each operand 14 words).  The first
    SUBSET_LEN entries hold every class (the partial-wave geometry runs those).  No case occurs twice, so every wave of a run
    holds 64 different cases (the asm blocks clobber vcc per statement)."""
    name, args = op
    rnd = random.Random("%d %s %r" % (seed, name, args))
    b = op_bounds(op)
    if name == "from_fp":
        vals = FP_EDGES + top_limb_family(rnd, 6) + [rnd.randrange(P) for _ in range(RANDOM_FILL)]
        return [([(v >> (32 * j)) & 0xffffffff for j in range(12)] + [0, 0],) for v in vals]
    worst = [[operand_worst(*bd) for bd in b]]
    for i in range(len(b)):      # each operand at its worst against mixes of the others
        if len(b) > 1:
            worst.append([operand_worst(*bd) if j == i else operand_mix(rnd, *bd) for j, bd in enumerate(b)])
    mixes = [[operand_mix(rnd, *bd) for bd in b] for _ in range(64)]
    edge_lists = [operand_edges(rnd, *bd) for bd in b]
    edges = []
    n_edge = max(len(e) for e in edge_lists)
    if len(b) == 1:
        edges = [[e] for e in edge_lists[0]]
    else:
        for k in range(n_edge * n_edge if len(b) == 2 else 4 * n_edge):
            edges.append([e[(k // n_edge ** (i % 2)) % len(e)] if i < 2 else e[(k * (i + 2) + i) % len(e)]
                          for i, e in enumerate(edge_lists)])
    rnd.shuffle(edges)           # the head of the list (the partial-wave subset) then spans both operands' edges
    quot = _quotient_cases(rnd, op) if name in ("mul", "sqr", "mul_add2") else []
    fill = [[operand_random(rnd, *bd) for bd in b] for _ in range(RANDOM_FILL)]
    extra = []
    if name == "equal":          # equal residues in different representations, and their neighbours
        (LA, VA), (LB, VB) = b
        for k in range(40):
            av = rnd.randrange(VA * P + 1) if k else 0
            a = canonical_limbs(av)
            j = rnd.randrange(VB) if VB > 1 else 0
            bv = av % P + j * P
            extra.append([a, canonical_limbs(bv)])
            extra.append([a, canonical_limbs(bv + 1 if bv + 1 <= VB * P else bv - 1)])
    if name == "is_zero":
        extra = [[canonical_limbs(v)] for v in (0, P, 1, P - 1, P + 1, 2 * P - 1, 1 << 364, P_LIMBS[13] << 364)]
    if name == "cneg":
        def reduced(c):
            return [canonical_limbs(value(c[0]) % P) if value(c[0]) >= P else c[0]]
        allc = [reduced(c) for c in worst + mixes + edges + fill]
        return [tuple(c) for c in _unique([c + [[neg] + [0] * 13] for c in allc for neg in (0, 1)])]
    if name == "is_zero":        # its contract is a Montgomery product: strictly below 2p
        keep = lambda cs: [c for c in cs if value(c[0]) < 2 * P]
        worst, mixes, edges, fill = keep(worst), keep(mixes), keep(edges), keep(fill)
    head = _unique(worst + quot + extra + mixes[:16] + edges[:40])
    nf = max(0, SUBSET_LEN - len(head))
    return [tuple(c) for c in _unique(head + fill[:nf] + mixes[16:] + edges[40:] + fill[nf:])]


SUBSET_LEN = 101


def mont_reference(op, operands):
    """(exact 14-word result, peak of the column accumulator) of a Montgomery routine on `operands`, after the
    column walk has been replayed and found below 2^64"""
    name = op[0]
    if name == "mul":
        pairs = [(operands[0], operands[1])]
    elif name == "sqr":
        pairs = [(operands[0], operands[0])]
    else:
        pairs = [(operands[0], operands[1]), (operands[2], operands[3])]
    t, _ = mont_exact(pairs)
    assert t < 2 * P
    want = canonical_limbs(t)
    walked, peak = replay_columns(pairs, square=(name == "sqr"))
    assert peak < 1 << 64, "the header's bound is wrong: column accumulator reaches %x" % peak
    assert walked == want and all(l <= M28 for l in want[:13])
    return want, peak


def check_field_result(op, operands, out):
    """assert that `out` (14 words) is what the operation must return for `operands`; returns the peak of the
    column accumulator for the Montgomery routines (else 0)"""
    name, args = op
    out = [int(x) for x in out]
    vals = [value(o) for o in operands]
    if name in ("mul", "sqr", "mul_add2"):
        want, peak = mont_reference(op, operands)
        assert all(l <= M28 for l in out[:13]) and out == want, (op, operands, out, want)
        return peak
    if name == "add":
        assert out == [x + y for x, y in zip(operands[0], operands[1])], (op, operands, out)
    elif name in ("sub", "sub_k"):
        if name == "sub":
            LA, VA, LB, VB = args
            K = 1
            while K <= VB:
                K <<= 1
        else:
            K, LA, VA, LB, VB = args
        assert all(l < (LA + LB + 2) << 28 for l in out), (op, operands, out)
        assert value(out) == vals[0] + K * P - vals[1], (op, operands, out)
    elif name == "norm":
        assert all(l <= M28 for l in out[:13]) and value(out) == vals[0], (op, operands, out)
    elif name == "to_fp":
        got = sum(out[j] << (32 * j) for j in range(12))
        assert got == vals[0] * pow(2, -8, P) % P and out[12:] == [0, 0], (op, operands, out)
    elif name == "from_fp":
        x = sum(operands[0][j] << (32 * j) for j in range(12))
        t, _ = mont_exact([(canonical_limbs(x), canonical_limbs(pow(2, 400, P)))])
        assert out == canonical_limbs(t) and t < 2 * P and t % P == x * 256 % P, (op, operands, out)
    elif name == "cneg":
        neg = operands[1][0]
        assert all(l < 4 << 28 for l in out) and value(out) == (2 * P - vals[0] if neg else vals[0]), (op, operands, out)
        if not neg:
            assert out == list(operands[0])
    elif name == "is_zero":
        assert out[0] == (1 if vals[0] % P == 0 else 0) and not any(out[1:]), (op, operands, out)
    elif name == "equal":
        assert out[0] == (1 if (vals[0] - vals[1]) % P == 0 else 0) and not any(out[1:]), (op, operands, out)
    else:
        raise ValueError(name)
    return 0


# ---- group-law scripts (the corpora of test_host_arith.py, consumed by the device tests too) ----

DBL_CHAIN_LENGTHS = [1, 2, 5, 64, 131, 300]

# (a, b, negate b) by name: the six special-case tuples of jac28_add
JAC_ADD_TUPLES = [("p1", "p2", 0), ("p1", "p2", 1), ("p1", "p1", 0), ("p1", "p1", 1), ("inf", "p2", 0), ("inf", "p2", 1)]


def alternation_scripts(rnd, nbase=12):
    """(index into a list of nbase points, subtract?) scripts for xyzz28_madd_alt: first point, doubling as a later
    addition, cancellation to infinity, restart, long chains; ("dbl", script) appends the running sum itself"""
    scripts = [
        [(0, 0)], [(0, 1)], [(0, 0), (1, 0)], [(0, 1), (1, 0)], [(0, 0), (1, 1), (2, 0)],
        [(0, 0), (0, 0)], [(0, 1), (0, 1)],                       # doubling as 2nd addition (stored sign "-")
        [(0, 0), (1, 0), (0, 0)],
        [(0, 0), (0, 1)], [(0, 1), (0, 0), (3, 0)],               # cancel, then restart
        [(0, 0), (1, 0), (1, 1), (0, 1), (2, 1), (3, 0)],         # cancel in the middle of a chain
        [(i % nbase, rnd.randrange(2)) for i in range(150)],
        [(rnd.randrange(nbase), rnd.randrange(2)) for i in range(200)],
    ]
    # P + Q where P = acc exactly (doubling at a later, even/odd position)
    for pos in (2, 3):
        sc = [(i, 0) for i in range(pos)]
        scripts.append(("dbl", sc))
    return scripts


W4_SCALARS = [0, 1, 15, 16, R - 1, R]
ORDER3_SCALARS = [3, 6, 7, R, R + 1, 4]


def glv_scalars(rnd):
    """the lambda-adjacent scalars, twiddle powers w^(64 i) and random fill of test_glv_split_and_glv_scalar_mul"""
    w = pow(7, (R - 1) // 8192, R)
    ks = [0, 1, LAMBDA - 1, LAMBDA, LAMBDA + 1, R - 1, R - 2, 2 ** 128, 2 ** 128 - 1, LAMBDA * LAMBDA, LAMBDA * LAMBDA + LAMBDA]
    ks += [pow(w, 64 * i, R) for i in range(0, 129, 7)] + [rnd.randrange(R) for _ in range(40)]
    return ks


HALF_SCALARS = [0, 1, 15, 16, 2 ** 127, 2 ** 128 - 1]
# Small k.  The w4_128 quad ladder reaches the doubling fallback of its addition while it BUILDS its table (P + P);
# inside a ladder over a point of the prime-order subgroup a partial sum never meets a table entry, whatever k is.
# The fallbacks are otherwise reached directly (test_additions) and on the non-subgroup corpus of the subgroup test.
SELF_MEETING_SCALARS = [2, 3, 6, 14]


# ---- the plain NAF of the pipelined ladders (naf2_128, naf_masks) ----

NAF2_LEN = 130


def naf_scalars():
    """128-bit values for naf2_128: the half-scalar edges (2^128 - 1 carries into the fifth word), small values, long
    carry runs, both halves of every scalar of glv_scalars() (the twiddle powers among them) and random halves"""
    rnd = random.Random(4005)
    full = glv_scalars(random.Random(29))
    ks = HALF_SCALARS + SELF_MEETING_SCALARS + [2 ** 128 - 2, 2 ** 127 - 1, 2 ** 127 + 1, 2 ** 64 - 1, 2 ** 64, 2 ** 96 - 1,
                                                 (2 ** 128 - 1) // 3, 2 * (2 ** 128 - 1) // 3, 3 << 126]
    ks += [k % LAMBDA for k in full] + [k // LAMBDA for k in full]
    ks += [rnd.randrange(1 << 128) for _ in range(60)] + [rnd.randrange(1 << rnd.randrange(1, 128)) for _ in range(20)]
    assert all(0 <= k < 1 << 128 for k in ks)
    return ks


def check_naf2(k, digits):
    """`digits` is THE non-adjacent form of k: NAF2_LEN digits in {0, +-1} that sum to k, no two adjacent non-zero
    (the form with these properties is unique)"""
    digits = [int(d) for d in digits]
    assert len(digits) == NAF2_LEN and all(d in (-1, 0, 1) for d in digits), (k, digits)
    assert sum(d << i for i, d in enumerate(digits)) == k, (k, digits)
    assert not any(digits[i] and digits[i + 1] for i in range(NAF2_LEN - 1)), (k, digits)


def naf_masks_expected(d1, d2):
    """naf_masks of two digit strings as 13 integers: nz[0][0..2] neg[0][0..2] nz[1][0..2] neg[1][0..2] top"""
    out = []
    for d in (d1, d2):
        nz = sum(1 << i for i, x in enumerate(d) if x)
        ng = sum(1 << i for i, x in enumerate(d) if x < 0)
        out += [(nz >> (64 * w)) & (2 ** 64 - 1) for w in range(3)] + [(ng >> (64 * w)) & (2 ** 64 - 1) for w in range(3)]
    top = max([i for i in range(NAF2_LEN) if d1[i] or d2[i]], default=-1)
    return out + [top]


def curve_point_xy(x0):
    """the first curve point (x, y) with x >= x0, affine integers"""
    x = x0
    while True:
        rhs = (x * x * x + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return x, y
        x += 1


# ---- running a field corpus through a shim's raw-limb entry point ----

_FIELD_REFERENCE = {}


def field_reference(op):
    """(cases, expected) for one operation, computed once per process: expected[i] is the exact 14-word result for
    the Montgomery routines (after the column walk has been replayed and found below 2^64) and None where
    check_field_result() states the property instead; third value: the largest column accumulator met"""
    if op not in _FIELD_REFERENCE:
        cases = field_cases(op)
        wants, peak = [], 0
        for c in cases:
            if op[0] in ("mul", "sqr", "mul_add2"):
                want, pk = mont_reference(op, c)
                peak = max(peak, pk)
                wants.append(want)
            else:
                wants.append(None)
        _FIELD_REFERENCE[op] = (cases, wants, peak)
    return _FIELD_REFERENCE[op]


def check_field_run(op, out, count=None):
    """the first `count` items (default: all) of a shim's output for field_reference(op)'s cases"""
    cases, wants, _ = field_reference(op)
    n = len(cases) if count is None else count
    out = list(out)
    for i in range(n):
        got = out[14 * i:14 * i + 14]
        if wants[i] is not None:
            assert got == wants[i], (op, i, cases[i], got, wants[i])
        else:
            check_field_result(op, cases[i], got)


def pack_operands(cases):
    """cases -> four ctypes arrays of n * 14 words (operands an operation does not take are zero)"""
    import ctypes as C
    n = len(cases)
    bufs = []
    for k in range(4):
        flat = []
        for c in cases:
            flat.extend(c[k] if k < len(c) else [0] * 14)
        bufs.append((C.c_uint32 * (14 * n))(*flat))
    return bufs
