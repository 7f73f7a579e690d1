"""The exact reference of Fp on 13 signed 30-bit limbs (c-kzg-4844_amd/csrc/fp30.hpp) and of the accumulate loop's
mixed addition on it (g1_30.hpp), in plain Python integers, and the deterministic corpora that tests/test_fp30_cpu.py
(the host build, hs_f30_run / hs_madd30_step / ...) and tests/test_gpu_fp30.py (the device builds, ds_plain_* /
ds_asm_*) both run.  Everything is compared limb for limb: no tolerance, no reduction mod p first.

Models.  A Montgomery product is model_product(s): (s + q p) / 2^390 with the balanced quotient, cut into balanced
limbs; column_product() is the column walk itself and asserts the signed 64-bit budget of every column.  norm, unpack
and to_f28 are written from fp30.hpp; madd_step, phi_step and exit_step from the formulas in g1_30.hpp's header
comment, with model_product for every product.  tests/test_fp30_cpu.py anchors the step model to the CPU oracle's
group law, independently of the code under test.

Corpora (field_cases(op), cached).  Every item carries a class name; items are interleaved so that each class is among
the first SUBSET_LEN.  Classes: random operands at the declared bounds; extreme_operands() crossed; named values (0,
+-1, +-p, +-vb p, 2^390 mod p, p +- 1 where the bound admits them); fullest columns (limbs 0..11 all at +-2^29 and the
alternations, for mul_add2 with both products aligned in sign); result digits at both ends of their range in every
column 0..11 ("rdigit": b solved from a target result, asserted from the model); quotient digits 0..11 at both ends of
their range ("qdigit": b chosen one column at a time, coverage asserted from the model).  Quotient digit 12 and result
limb 12 are left to the random and extreme cases: nothing here steers them and nothing is claimed about them."""
import random

from arith_cases import LAMBDA, P, R

N, W = 13, 30
HALF = 1 << 29
MASK = (1 << W) - 1
H13 = sum(HALF << (W * j) for j in range(N))        # value of the digit string (2^29, ..., 2^29), 13 digits
H12 = sum(HALF << (W * j) for j in range(N - 1))
PINV390 = pow(P, -1, 1 << 390)
R390 = pow(2, 390, P)
SUBSET_LEN = 101
STATE_WORDS, ENTRY_WORDS, EXIT_WORDS = 52, 24, 56


def value(limbs):
    return sum(int(v) << (W * j) for j, v in enumerate(limbs))


def out_limbs(v):
    """what a product or norm() leaves: limbs 0..11 balanced in [-2^29, 2^29), limb 12 the rest"""
    low = ((v + H12) % (1 << 360)) - H12
    t = low + H12
    return [((t >> (W * j)) & ((1 << W) - 1)) - HALF for j in range(N - 1)] + [(v - low) >> 360]


def quotient_digits(s):
    """the 13 balanced quotient digits of a product sum s: q = -s/p mod 2^390, digits in [-2^29, 2^29)"""
    q = (((-s * PINV390) % (1 << 390)) + H13) % (1 << 390)
    return [((q >> (W * j)) & MASK) - HALF for j in range(N)]


def model_product(s):
    """(s + q p) / 2^390 with the balanced quotient q = -s/p mod 2^390, digits in [-2^29, 2^29)"""
    q = (((-s * PINV390) % (1 << 390)) + H13) % (1 << 390) - H13
    t = s + q * P
    assert t % (1 << 390) == 0
    return out_limbs(t >> 390)


def column_product(a, b, c=None, d=None):
    """the column walk itself, digit by digit (checks model_product, and the 64-bit bound of every column)"""
    pl = out_limbs(P)
    ninv = (-pow(P, -1, 1 << W)) % (1 << W)
    q, r, acc = [], [], 0
    for k in range(2 * N - 1):
        lo, hi = max(0, k - (N - 1)), min(k, N - 1)
        acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        if c is not None:
            acc += sum(c[i] * d[k - i] for i in range(lo, hi + 1))
        up = 0
        if c is not None and 10 <= k <= 14:
            assert abs(acc) < 1 << 63
            up, acc = acc >> W, acc & ((1 << W) - 1)
        acc += sum(q[i] * pl[k - i] for i in range(lo, min(hi, len(q) - 1) + 1) if k - i >= 1)
        if k < N:
            qk = ((acc * ninv) % (1 << W) + HALF) % (1 << W) - HALF
            q.append(qk)
            acc += qk * pl[0]
        else:
            r.append(((acc % (1 << W)) + HALF) % (1 << W) - HALF)
            acc -= r[-1]
        assert abs(acc) < (1 << 63) - (1 << 60), k     # 2^60: room for the carry bias of two columns
        assert acc % (1 << W) == 0
        acc = (acc >> W) + up
    return r + [acc]


def rand_operand(rnd, vb):
    """normalised limbs of a random value of magnitude <= vb p"""
    return out_limbs(rnd.randrange(-vb * P, vb * P + 1))


def extreme_operands(vb):
    """the declared bounds, both signs: values at +-vb p, and limbs 0..11 all at +-2^29 (alternating too) under
    a top limb that keeps the value inside +-vb p"""
    out = [out_limbs(vb * P), out_limbs(-vb * P), [0] * N]
    for pattern in ([HALF] * 12, [-HALF] * 12, [HALF, -HALF] * 6, [-HALF, HALF] * 6):
        for target in (vb * P, -vb * P, 0):
            top = (target - value(pattern)) >> 360
            for t in (top, top + 1):
                cand = pattern + [t]
                if abs(value(cand)) <= vb * P and abs(t) <= HALF:
                    out.append(cand)
    assert len(out) >= 10
    return out


# ---- limb-exact models of the routines that are not products ----

def sext30(v):
    return ((v & MASK) + HALF) % (1 << W) - HALF


def model_norm(limbs, la, va):
    """norm<LA, VA>: the corpus must keep every intermediate inside 32 bits, as the static_asserts promise"""
    assert all(abs(v) <= la * HALF for v in limbs[:12]), limbs
    assert abs(limbs[12]) <= (va << 21) + 1, limbs
    r = out_limbs(value(limbs))
    assert abs(r[12]) < 1 << 31
    return r


def model_unpack(words):
    """f30_unpack: field j sign-extended, plus bit 29 of the field below; a limb may be +2^29"""
    v = sum(int(w) << (32 * i) for i, w in enumerate(words))
    assert 0 <= v < P
    f = [(v >> (W * j)) & MASK for j in range(N)]
    r = []
    for j in range(N):
        s = sext30(f[j]) if j < 12 else f[j]
        r.append(s if j == 0 else s + ((f[j - 1] >> 29) & 1))
    assert value(r) == v
    return r


def model_to_f28(limbs):
    """f30_to_f28: value + p in 14 limbs of 28 bits (the top one takes the rest)"""
    v = value(limbs)
    assert abs(v) <= P and all(abs(x) <= HALF for x in limbs)
    v += P
    return [(v >> (28 * j)) & ((1 << 28) - 1) for j in range(13)] + [v >> 364]


PL = out_limbs(P)
NINV = (-pow(P, -1, 1 << W)) % (1 << W)
R392L = out_limbs(pow(2, 392, P))
R394L = out_limbs(pow(2, 394, P))


# ---- the curve, in affine integers (corpus construction only; the oracle is the tests' reference) ----

GX = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
GY = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1
assert (GY * GY - GX ** 3 - 4) % P == 0


def ec_add(a, b):
    """affine points as (x, y), None for infinity"""
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def ec_neg(a):
    return None if a is None else (a[0], -a[1] % P)


def ec_mul(a, k):
    r = None
    while k:
        if k & 1:
            r = ec_add(r, a)
        a = ec_add(a, a)
        k >>= 1
    return r


_BETA = []


def beta():
    """the cube root of unity with (beta x, y) = LAMBDA (x, y), found on the curve: independent of the headers"""
    if not _BETA:
        lg = ec_mul((GX, GY), LAMBDA)
        assert lg[1] == GY
        b = lg[0] * pow(GX, -1, P) % P
        assert b != 1 and pow(b, 3, P) == 1
        _BETA.append(b)
    return _BETA[0]


def beta390_limbs():
    return out_limbs(beta() * R390 % P)


def entry_words(pt):
    """a table entry as the kernel gathers it: x, y in the 2^392 domain, fully reduced, 12 packed words each"""
    out = []
    for v in pt:
        t = v * pow(2, 392, P) % P
        out += [(t >> (32 * i)) & 0xffffffff for i in range(12)]
    return out


# ---- the addition: g1_30.hpp's header comment, with model_product for every product ----

def _bounded(limbs, vb):
    assert all(abs(v) <= HALF for v in limbs) and abs(value(limbs)) <= vb * P, (limbs, vb)
    return value(limbs)


def check_state(state):
    """the declared bounds of an XYZZ30: x <1,4>, w, zz, zzz <1,1>"""
    x, w, zz, zzz = state
    return _bounded(x, 4), _bounded(w, 1), _bounded(zz, 1), _bounded(zzz, 1)


def _prod(s, *bounds):
    """a product whose operands' value bounds multiply to at most 314: comes out at most p in magnitude"""
    r = model_product(s)
    assert abs(value(r)) <= P and all(-HALF <= v < HALF for v in r[:12]) and abs(r[12]) <= HALF
    return r


def madd_step(state, inf, yneg, words, dneg):
    """xyzz30_madd_alt: (state, inf, yneg) after adding +-(the entry); state = [x, w, zz, zzz] as limb lists"""
    x2, y2 = model_unpack(words[:12]), model_unpack(words[12:])
    if inf:
        yneg = False
    tneg = dneg != (not yneg)
    t = [-v for v in y2] if tneg else y2
    if inf:
        return [_prod(value(x2) * value(R392L)), _prod(value(t) * value(R394L)), list(R392L), list(R394L)], False, True
    X, Wv, ZZ, ZZZ = check_state(state)
    u2 = _prod(value(x2) * ZZ)
    tt = _prod(value(t) * ZZZ)
    p = model_norm([a - b for a, b in zip(u2, state[0])], 2, 5)
    r = model_norm([a + b for a, b in zip(tt, state[1])], 2, 2)
    pp = _prod(value(p) ** 2)
    ppp = _prod(value(p) * value(pp))
    q = _prod(X * value(pp))
    rr = _prod(value(r) ** 2)
    t1 = model_norm([a + 2 * b for a, b in zip(ppp, q)], 3, 3)
    x3 = model_norm([a - b for a, b in zip(rr, t1)], 2, 4)
    d = model_norm([a - b for a, b in zip(q, x3)], 2, 5)
    w3 = _prod(value(r) * value(d) + Wv * value(ppp))
    zz3 = _prod(ZZ * value(pp))
    zzz3 = _prod(ZZZ * value(ppp))
    return [x3, w3, zz3, zzz3], False, not yneg


def phi_step(state):
    X = check_state(state)[0]
    return [_prod(X * value(beta390_limbs()))] + [list(v) for v in state[1:]]


def exit_step(state):
    """xyzz30_to_xyzz28 (56 words) and xyzz30_met_equal_x"""
    X, Wv, ZZ, ZZZ = check_state(state)
    r392, r394 = value(R392L), value(R394L)
    parts = [model_to_f28(_prod(X * r392)), model_to_f28(_prod(Wv * r392)), model_to_f28(_prod(ZZ * r394)),
             model_to_f28(_prod(ZZZ * r394))]
    zz = sum(v << (28 * j) for j, v in enumerate(parts[2]))
    assert 0 <= zz <= 2 * P
    return [w for part in parts for w in part], 1 if zz in (0, P) else 0


def state_point(state, yneg):
    """the affine point an accumulator stands for, read through the weights (1, 2, 0, 1) and the sign flag; None when
    ZZ = 0 mod p (no point: some step met equal x)"""
    X, Wv, ZZ, ZZZ = (value(v) for v in state)
    if ZZ % P == 0:
        return None
    k = 4
    zz, zzz = ZZ, ZZZ * pow(k, -1, P)                     # both times 2^392, which cancels below
    x = X * pow(k, -1, P) * pow(zz, -1, P) % P
    y = Wv * pow(k * k, -1, P) * pow(zzz, -1, P) % P
    return x, (-y % P if yneg else y)


# ---- corpora ----

def parse_ops(desc):
    """f30test::desc() -> [(name, (template arguments))]"""
    ops = []
    for line in desc.strip().split("\n"):
        parts = line.split()
        ops.append((parts[0], tuple(int(v) for v in parts[1:])))
    return ops


REQUIRED_OPS = [("mul", (1, 1)), ("mul", (5, 1)), ("mul", (4, 1)), ("mul", (17, 18)), ("sqr", (5,)), ("sqr", (2,)),
                ("sqr", (17,)), ("mul_add2", (2, 5, 1, 1)), ("mul_add2", (17, 17, 5, 5)), ("norm", (1, 1)),
                ("norm", (2, 5)), ("norm", (2, 2)), ("norm", (2, 4)), ("norm", (3, 3)), ("norm", (3, 200)),
                ("add", (1, 1, 1, 1)), ("add", (1, 1, 2, 2)), ("sub", (1, 1, 1, 4)), ("sub", (1, 1, 1, 3)),
                ("neg", (1,)), ("unpack", ()), ("to_f28", ()), ("const", ())]
PRODUCTS = ("mul", "sqr", "mul_add2")
PATTERNS = ([HALF] * 12, [-HALF] * 12, [HALF, -HALF] * 6, [-HALF, HALF] * 6)
DIGIT_TARGETS = ([-HALF] * 12, [HALF - 1] * 12, [-HALF, HALF - 1] * 6, [HALF - 1, -HALF] * 6)
RANDOM_FILL = 300


def named_values(vb):
    vals = [0, 1, -1, P, -P, vb * P, -vb * P, R390, P + 1, P - 1, -(P + 1), -(P - 1)]
    out = []
    for v in vals:
        if abs(v) <= vb * P and v not in out:
            out.append(v)
    return [out_limbs(v) for v in out]


def _balanced30(v):
    return (v + HALF) % (1 << W) - HALF


def _steer_quotient(a, rest):
    """b with limbs 0..11 chosen one column at a time so that quotient digits 0..11 of a * b + rest equal each of
    DIGIT_TARGETS in turn: q_k moves by -a_0 b_k / p_0, so b_k = -(target_k - q_k) p_0 / a_0 mod 2^30, balanced"""
    assert a[0] & 1
    inv = PL[0] * pow(a[0], -1, 1 << W)
    out = []
    for target in DIGIT_TARGETS:
        b = [0] * N
        for k in range(12):
            qk = quotient_digits(value(a) * value(b) + rest)[k]
            b[k] = _balanced30(-(target[k] - qk) * inv)
        assert quotient_digits(value(a) * value(b) + rest)[:12] == list(target)
        out.append(b)
    return out


def _result_targets():
    return [list(t) + [top] for t in DIGIT_TARGETS for top in (0, 1, -1, 1 << 19, -(1 << 19))]


def _unit(rnd):
    v = rnd.randrange(1, P)
    return v if rnd.randrange(2) else -v


def _odd_operand(rnd, vb):
    """a random operand at the bound whose limb 0 is odd (a unit mod 2^30)"""
    while True:
        a = rand_operand(rnd, vb)
        a[0] |= 1
        if abs(value(a)) <= vb * P:
            return a


def _product_cases(op, rnd):
    name, vb = op
    cls = {}
    if name == "mul":
        va, vbb = vb
        cls["random"] = [(rand_operand(rnd, va), rand_operand(rnd, vbb)) for _ in range(RANDOM_FILL)]
        cls["extreme"] = [(a, b) for b in extreme_operands(vbb) for a in extreme_operands(va)]
        cls["named"] = [(a, b) for a in named_values(va) for b in named_values(vbb)]
        cls["full"] = [(x + [0], [s * v for v in y] + [0]) for x in PATTERNS for y in PATTERNS for s in (1, -1)]
        cls["rdigit"] = []
        for t in _result_targets():
            a = _unit(rnd)
            b = value(t) * R390 * pow(a, -1, P) % P
            cls["rdigit"].append((out_limbs(a), out_limbs(b), t))
        cls["qdigit"] = []
        for _ in range(6):
            a = _odd_operand(rnd, va)
            cls["qdigit"] += [(a, b) for b in _steer_quotient(a, 0)]
    elif name == "sqr":
        va, = vb
        cls["random"] = [(rand_operand(rnd, va),) for _ in range(RANDOM_FILL)]
        cls["extreme"] = [(a,) for a in extreme_operands(va)]
        cls["named"] = [(a,) for a in named_values(va)]
        cls["full"] = [(x + [0],) for x in PATTERNS]
        cls["rdigit"] = []
        for t in _result_targets():
            sq = value(t) * R390 % P
            a = pow(sq, (P + 1) // 4, P)
            if a * a % P == sq:                       # half of the targets have a root; the coverage is asserted below
                cls["rdigit"] += [(out_limbs(a), t), (out_limbs(-a), t)]
    else:
        va, vbb, vc, vd = vb
        cls["random"] = [tuple(rand_operand(rnd, v) for v in vb) for _ in range(RANDOM_FILL)]
        ea, eb, ec, ed = (extreme_operands(v) for v in vb)
        cls["extreme"] = [(ea[k % len(ea)], eb[(k // len(ea)) % len(eb)], ec[k % len(ec)], ed[(k // 3) % len(ed)])
                          for k in range(len(ea) * len(eb))]
        na, nb, nc, nd = (named_values(v) for v in vb)
        cls["named"] = [(a, b, nc[(i + j) % len(nc)], nd[(i * j) % len(nd)]) for i, a in enumerate(na) for j, b in enumerate(nb)]
        cls["full"] = []
        for x in PATTERNS:
            for y in PATTERNS:
                for s in (1, -1):
                    fx, fy = x + [0], [s * v for v in y] + [0]
                    cls["full"].append((fx, fy, fx, fy))                               # both products aligned in sign
                    cls["full"].append((fx, fy, fy, fx))
                    cls["full"].append((fx, fy, [-v for v in fx], fy))                 # and opposed: the columns cancel
        cls["rdigit"] = []
        for t in _result_targets():
            a, c, d = _unit(rnd), _unit(rnd), _unit(rnd)
            b = (value(t) * R390 - c * d) * pow(a, -1, P) % P
            cls["rdigit"].append((out_limbs(a), out_limbs(b), out_limbs(c), out_limbs(d), t))
        cls["qdigit"] = []
        for _ in range(6):
            a, c, d = _odd_operand(rnd, va), rand_operand(rnd, vc), rand_operand(rnd, vd)
            cls["qdigit"] += [(a, b, c, d) for b in _steer_quotient(a, value(c) * value(d))]
    return cls


def product_sum(name, ops):
    if name == "mul":
        return value(ops[0]) * value(ops[1])
    if name == "sqr":
        return value(ops[0]) ** 2
    return value(ops[0]) * value(ops[1]) + value(ops[2]) * value(ops[3])


def _split(la, va):
    """value bounds of the LA normalised operands whose sum a norm<LA, VA> input is"""
    parts = [va // la] * la
    parts[-1] += va - sum(parts)
    return parts


def _norm_cases(la, va, rnd):
    cls = {}
    parts = _split(la, va)
    signs = [[1] * la, [1] + [-1] * (la - 1), [-1] * la]
    cls["random"] = []
    for k in range(RANDOM_FILL):
        sg = signs[k % len(signs)]
        xs = [rand_operand(rnd, v) for v in parts]
        cls["random"].append([sum(s * x[j] for s, x in zip(sg, xs)) for j in range(N)])
    cls["extreme"] = []
    ex = [extreme_operands(v) for v in parts]
    for k in range(max(len(e) for e in ex) * 3):
        sg = signs[k % len(signs)]
        xs = [e[(k // (i + 1)) % len(e)] for i, e in enumerate(ex)]
        cls["extreme"].append([sum(s * x[j] for s, x in zip(sg, xs)) for j in range(N)])
    # every limb at +-LA 2^29 (and alternating), under top limbs at the value bound and at the VA 2^21 of the header
    cls["limb_bound"] = []
    vtop = (va * P) >> 360
    for pat in ([1] * 12, [-1] * 12, [1, -1] * 6, [-1, 1] * 6):
        for top in (vtop - 1, -vtop + 1, va << 21, -(va << 21), 0):
            cls["limb_bound"].append([s * la * HALF for s in pat] + [top])
    # carries that ripple through all twelve limbs
    cls["ripple"] = []
    for top in (0, vtop - 1, -vtop + 1):
        cls["ripple"].append([HALF] + [HALF - 1] * 11 + [top])               # (2^29 - 1, ...) plus one in limb 0
        cls["ripple"].append([HALF] * 12 + [top])                            # admitted at LA = 1 too: |limb| <= 2^29
        if la >= 2:
            cls["ripple"].append([-HALF - 1] + [-HALF] * 11 + [top])         # the negative mirror
            cls["ripple"].append([la * HALF] + [la * HALF - 1] * 11 + [top])     # the same at the limb bound: the
            cls["ripple"].append([-la * HALF] * 12 + [top])                      # carry is 2 (-2) at LA = 3
    for x in cls["ripple"]:
        carries, c = [], 0
        for v in x[:12]:
            c = (v + c - sext30(v + c)) >> W
            carries.append(c)
        assert all(carries), x                                               # a carry leaves every limb
    return {k: [(v,) for v in vs] for k, vs in cls.items()}


def _lazy_operand(rnd, la, va, k):
    """an operand of limb bound la: the sum of la normalised ones"""
    parts = _split(la, va)
    if k % 3 == 0:
        xs = [extreme_operands(v)[(k // 3 + i) % len(extreme_operands(v))] for i, v in enumerate(parts)]
    else:
        xs = [rand_operand(rnd, v) for v in parts]
    return [sum(x[j] for x in xs) for j in range(N)]


def _unpack_values(rnd):
    edge = [0, 1, P - 1, P - 2, sum(1 << (W * j + 29) for j in range(12)),
            sum(MASK << (W * j) for j in range(12)), sum((HALF - 1) << (W * j) for j in range(12))]
    for top in (0, 1, (1 << 20) - 1):            # bit 29 of every 30-bit field set, other bits random
        for _ in range(4):
            edge.append(sum((HALF | rnd.randrange(HALF)) << (W * j) for j in range(12)) + (top << 360))
    return edge + [rnd.randrange(P) for _ in range(RANDOM_FILL)]


def _to_f28_cases(rnd):
    vals = [P, -P, P - 1, -(P - 1), 0, 1, -1, (1 << 360) - P, (1 << 360) - 1 - P, (1 << 380) - P, -(1 << 360)]
    out = [out_limbs(v) for v in vals]
    out.append([-1 - PL[0]] + [-v for v in PL[1:12]] + [1 - PL[12]])      # + p borrows through every field
    out.append([-PL[0]] + [-v for v in PL[1:12]] + [-PL[12]])            # -p in the limbs of -F30_P
    out += [x for x in extreme_operands(1)]
    return [(x,) for x in out + [rand_operand(rnd, 1) for _ in range(RANDOM_FILL)]]


def _interleave(cls):
    """one item of each class first, then round-robin: every class is among the first SUBSET_LEN"""
    assert len(cls) <= SUBSET_LEN
    out, k = [], 0
    while any(k < len(v) for v in cls.values()):
        for name in sorted(cls):
            if k < len(cls[name]):
                out.append((name, cls[name][k]))
        k += 1
    return out


_CASES = {}


def field_cases(op):
    """[(class, operands, expected 14 words)] for one operation of the list, computed once per process.  Operands are
    limb lists (unpack: 12 words); for the products the expected limbs come from model_product after column_product
    has walked the fullest columns inside the 64-bit budget."""
    if op in _CASES:
        return _CASES[op]
    name, args = op
    rnd = random.Random("f30 %s %s" % (name, args))
    out = []
    if name in PRODUCTS:
        seen_r = [set() for _ in range(12)]
        seen_q = [set() for _ in range(12)]
        for cl, item in _interleave(_product_cases(op, rnd)):
            ops = item[:{"mul": 2, "sqr": 1, "mul_add2": 4}[name]]
            for x, v in zip(ops, args):
                assert all(abs(l) <= HALF for l in x) and abs(value(x)) <= v * P, (op, cl, x)
            s = product_sum(name, ops)
            want = model_product(s)
            if cl == "full":
                got = column_product(ops[0], ops[0] if name == "sqr" else ops[1], *(ops[2:] if name == "mul_add2" else ()))
                assert got == want, (op, ops)
            if cl == "rdigit":
                assert want == item[-1], (op, item)          # the target comes out, from the model alone
            assert abs(value(want)) <= P and all(-HALF <= l < HALF for l in want[:12])
            for k in range(12):
                seen_r[k].add(want[k])
                seen_q[k].add(quotient_digits(s)[k])
            out.append((cl, ops, want + [0]))
        for k in range(12):
            assert {-HALF, HALF - 1} <= seen_r[k], (op, "result digit", k)
            if name != "sqr":
                assert {-HALF, HALF - 1} <= seen_q[k], (op, "quotient digit", k)
    elif name == "norm":
        for cl, (x,) in _interleave(_norm_cases(args[0], args[1], rnd)):
            out.append((cl, (x,), model_norm(x, *args) + [0]))
    elif name in ("add", "sub"):
        la, va, lb, vbb = args
        sg = 1 if name == "add" else -1
        for k in range(RANDOM_FILL):
            a, b = _lazy_operand(rnd, la, va, k), _lazy_operand(rnd, lb, vbb, k + 1)
            want = [x + sg * y for x, y in zip(a, b)]
            assert all(abs(v) < 1 << 31 for v in want)
            out.append(("extreme" if k % 3 == 0 else "random", (a, b), want + [0]))
    elif name == "neg":
        xs = extreme_operands(1) + [p + [0] for p in PATTERNS] + [rand_operand(rnd, 1) for _ in range(RANDOM_FILL)]
        out = [("neg", (x,), [-v for v in x] + [0]) for x in xs]
    elif name == "unpack":
        for v in _unpack_values(rnd):
            words = [(v >> (32 * i)) & 0xffffffff for i in range(12)]
            out.append(("unpack", (words + [0],), model_unpack(words) + [0]))
    elif name == "to_f28":
        out = [("to_f28", x, model_to_f28(x[0])) for x in _to_f28_cases(rnd)]
    elif name == "const":
        consts = [PL, R392L, R394L, beta390_limbs()]
        out = [("const", ([k] + [0] * 12,), consts[k] + [0]) for k in range(4)] + [("const", ([4] + [0] * 12,), [NINV] + [0] * 13)]
    else:
        raise AssertionError("no corpus for %s" % (op,))
    classes = {c for c, _, _ in out}
    assert classes == {c for c, _, _ in out[:SUBSET_LEN]}, (op, "a class is missing from the first items")
    _CASES[op] = out
    return out


def pack_field(cases):
    """four ctypes int32 arrays of n * 13 words (operands an operation does not take are zero)"""
    import ctypes as C
    n = len(cases)
    bufs = []
    for k in range(4):
        flat = []
        for _, ops, _ in cases:
            flat.extend([v - (1 << 32) if v >= 1 << 31 else v for v in ops[k]] if k < len(ops) else [0] * N)
        bufs.append((C.c_int32 * (N * n))(*flat))
    return bufs


def check_field(op, cases, out, count=None):
    """the first `count` results (14 int32 each) against the expected limbs; to_f28's words are unsigned"""
    n = len(cases) if count is None else count
    out = list(out)
    for i in range(n):
        got = out[14 * i:14 * i + 14]
        if op[0] in ("to_f28", "const"):
            got = [v & 0xffffffff for v in got]
            want = [v & 0xffffffff for v in cases[i][2]]
        else:
            want = cases[i][2]
        assert got == want, (op, i, cases[i][0], cases[i][1], got, want)
        if op[0] in PRODUCTS:
            assert abs(value(got[:13])) <= P and all(-HALF <= v < HALF for v in got[:12]), (op, i)


# ---- the addition's corpora ----

_STEP = {}


def corpus_points(n, seed=3030):
    """n points of the prime-order subgroup, affine integers"""
    rnd = random.Random(seed)
    return [ec_mul((GX, GY), rnd.randrange(1, R)) for _ in range(n)]


def _shifted(state):
    """the same point in other residues: X at +-4p, W, ZZ, ZZZ across zero by p"""
    out = []
    for sx in (1, -1):
        X = value(state[0])
        k = (4 * P - X) // P if sx > 0 else -((4 * P + X) // P)
        st = [out_limbs(X + k * P)]
        for j, v in enumerate(state[1:]):
            val = value(v)
            if sx < 0 and j == 1:
                st.append(list(v))                      # one of the two keeps ZZ as the step left it
            else:
                st.append(out_limbs(val + P if val <= 0 else val - P))
        for lim, vb in zip(st, (4, 1, 1, 1)):
            assert abs(value(lim)) <= vb * P
        out.append(st)
    return out


def step_cases():
    """[(class, state, inf, yneg, entry words, dneg, entry point, expected (state, inf, yneg))]: accumulators reached
    by modelled chains of 1, 2 and 50 steps, the same in shifted residues, the empty accumulator, both signs of the
    accumulator and of the entry, and an entry equal to the accumulator's point and to its negative"""
    if "step" in _STEP:
        return _STEP["step"]
    pts = corpus_points(60)
    rnd = random.Random(3031)
    states = []
    for length, first in ((1, 0), (2, 1), (50, 3), (1, 53), (3, 54)):
        st, inf, yneg = [[0] * N] * 4, True, False
        for i in range(length):
            st, inf, yneg = madd_step(st, inf, yneg, entry_words(pts[first + i]), rnd.randrange(2))
        states.append(("chain%d" % length, st, yneg))
        for sh in _shifted(st):
            states.append(("shifted%d" % length, sh, yneg))
    cases = []
    fresh = pts[57:60]
    for cl, st, yneg in states:
        for k, dneg in enumerate((0, 1)):
            cases.append((cl, st, 0, int(yneg), entry_words(fresh[k]), dneg, fresh[k]))
        own = state_point(st, yneg)
        cases.append(("equal_x", st, 0, int(yneg), entry_words(own), 0, own))          # doubling: not handled
        cases.append(("equal_x", st, 0, int(yneg), entry_words(own), 1, own))          # the negative
    garbage = [rand_operand(rnd, 1) for _ in range(4)]
    for st in ([[0] * N] * 4, garbage):
        for yneg in (0, 1):
            for dneg in (0, 1):
                cases.append(("empty", st, 1, yneg, entry_words(fresh[2]), dneg, fresh[2]))
    out = []
    for cl, st, inf, yneg, words, dneg, pt in cases:
        want = madd_step(st, bool(inf), bool(yneg), words, bool(dneg))
        if cl == "equal_x":
            assert value(want[0][2]) % P == 0
        out.append((cl, st, inf, yneg, words, dneg, pt, want))
    order = _interleave({c: [x for x in out if x[0] == c] for c in {x[0] for x in out}})
    _STEP["step"] = [x for _, x in order]
    return _STEP["step"]


def state_cases():
    """accumulators for phi30 and exit30: every input state of step_cases() that holds a point, and every state a
    step leaves -- those after an equal-x step included, where the exit must say so"""
    if "state" not in _STEP:
        out = []
        for cl, st, inf, _, _, _, _, want in step_cases():
            if not inf and st not in out:
                out.append(st)
            if want[0] not in out:
                out.append(want[0])
        assert any(exit_step(s)[1] for s in out) and not all(exit_step(s)[1] for s in out)
        _STEP["state"] = [(s, phi_step(s), exit_step(s)) for s in out]
    return _STEP["state"]


def flat_state(state):
    return [v for part in state for v in part]


def check_steps(steps, out, oflags, count=None):
    """a shim's madd30_step output against the model: 52 limbs and both flags per item"""
    n = len(steps) if count is None else count
    for i in range(n):
        want, inf, yneg = steps[i][7]
        assert out[STATE_WORDS * i:STATE_WORDS * (i + 1)] == flat_state(want), (i, steps[i][0])
        assert (oflags[2 * i], oflags[2 * i + 1]) == (int(inf), int(yneg)), (i, steps[i][0])


def check_states(states, phi_out, exit_out, met, count=None):
    """phi30's 52 limbs, exit30's 56 words and its verdict against the model"""
    n = len(states) if count is None else count
    for i in range(n):
        _, phi, (words, m) = states[i]
        assert phi_out[STATE_WORDS * i:STATE_WORDS * (i + 1)] == flat_state(phi), i
        assert exit_out[EXIT_WORDS * i:EXIT_WORDS * (i + 1)] == words, i
        assert met[i] == m, i


# ---- chains (points come from the caller's group: the CPU oracle) ----

def chain_300(grp, base_points, seed=34):
    """the chains of 300 entries of tests/test_fp30_cpu.py: (points, signs, at_inf) and the phi positions"""
    rnd = random.Random(seed)
    signs = [rnd.randrange(2) for _ in base_points]
    at_inf = [0] * len(base_points)
    for i in (0, 7, 150, 151, 299):
        at_inf[i] = 1                      # entries at infinity: first, in the middle, around phi, last
    return base_points, signs, at_inf, (151, 1, 300, 1000, 0)


def chain_expected(grp, pts, signs, at_inf, phi_at):
    """the chain's sum by the group law alone: phi is multiplication by LAMBDA"""
    run, pending = bytes(144), True
    for i, (p, s, z) in enumerate(zip(pts, signs, at_inf)):
        if pending and i >= phi_at:
            run, pending = grp.mul(run, LAMBDA), False
        if z:
            continue
        run = grp.add(run, grp.neg(p) if s else p)
    if pending:
        run = grp.mul(run, LAMBDA)
    return run


def equal_x_chains(grp, base_points, seed=35, head=11, tail=9):
    """acc + (its own point) and acc + (its negative), in the middle of a chain and as its last step"""
    rnd = random.Random(seed)
    signs = [rnd.randrange(2) for _ in range(head + tail)]
    run = bytes(144)
    for p, s in zip(base_points[:head], signs):
        run = grp.add(run, grp.neg(p) if s else p)
    out = []
    for same in (True, False):
        for rest in (tail, 0):
            cp = base_points[:head] + [grp.affine(run)] + base_points[head:head + rest]
            cs = signs[:head] + [0 if same else 1] + signs[head:head + rest]
            out.append((cp, cs, [0] * len(cp)))
    return out


def divergent_chains(grp, base_points, seed=36):
    """64 chains for one launch of 64 lanes: lengths 0, 1, 2 and up, one all at infinity, one with an equal-x step,
    each with a phi position of its own (before, inside, at and past its end)"""
    rnd = random.Random(seed)
    chains = []
    for c in range(64):
        length = c if c < 3 else rnd.randrange(3, 40)
        first = rnd.randrange(len(base_points) - 40)
        pts = base_points[first:first + length]
        signs = [rnd.randrange(2) for _ in pts]
        at_inf = [1 if rnd.randrange(8) == 0 else 0 for _ in pts]
        if c == 5:
            at_inf = [1] * length
        phi_at = [0, 1, length // 2, length, length + 7][c % 5]
        chains.append((pts, signs, at_inf, phi_at))
    eq = equal_x_chains(grp, base_points)[0]
    chains[9] = (eq[0], eq[1], eq[2], len(eq[0]) - 2)     # phi after the equal-x step: before it the sums would differ
    return chains
