"""The two length-128 G1 transforms at the end of the FK20 proofs (fk20.hip: fk20_fft_stage_enqueue) in Python integers.

A transform is 128 scalars a_f mod r -- the discrete logarithms of its points a_f * G -- and so is its output:

    out[k] = sum_{j < 64} w^(jk) * sum_{f < 128} w^(-fj) a_f,      w = W128

the inverse transform, its upper half dropped, the forward transform, with no factor 1/128 (the product folds that into
the MSM scalars).  `expect` computes it with two fast transforms, `expect_naive` straight from the formula.

The device runs the stage in one of three dataflows, chosen by the batch size (fk20_fft_plan.hpp), and each is replayed
here on discrete logarithms, addition by addition, in the order the kernels perform them:

    replay_r2   radix-2 stages: k_g1_fft_addsub per stage (u + v, u - v), the twiddle on the odd half, k_g1_fft_fold
    replay_r4   radix-4 pairs as the comment block above R4_LADDERS states them: the input combinations of
                k_g1_fft_r4_ladder, the five ladders of a group, the sums of k_g1_fft_r4_post; DIF (7,6) (5,4) (3,2), the
                fold, DIT (2,3) (4,5) (6,7)
    replay_r8   radix-8 triples as the block above R8_PER_GROUP states them: V(r, j) in the order r8_ladder_body and the
                doubler wave of r8_ladder_pipe_body accumulate it, the 21 ladders L(r, j) of a group, the sums of
                k_g1_fft_r8_post term by term; DIF (7,6,5) (4,3,2), k_g1_fft_fold_raw, DIT (2,3,4) (5,6,7)

A ladder is a multiplication by a power of w.  Every ADDITION is an event: its site (which addition of which kernel,
down to the term of a multi-term sum) and what it meets -- `plain`, `equal` (a doubling), `opposite` (the result is
the identity), `left` / `right` / `both` for an identity operand.  The G1 additions of the device take another path
for each of these (g1_quad.hpp: the quad forms fall back to the complete one-lane routine), which is why the corpus
below exists: vectors of scalars on which every kind of site meets every kind of operand pair.  tests/
test_fk20_expect_cpu.py counts that they do; tests/test_gpu_fk20_stages.py runs them on the device.

A replay can also keep the state after each step (`trace`: [(step, 128 scalars)]), the values a wrong device output is
walked back through."""
import random
from collections import Counter

from fk20_edge import R, W128

W = [pow(W128, e, R) for e in range(128)]
FORM_NAMES = ("r8_pipe_two", "r8_pipe", "r8_one", "r4", "r2_quad", "r2_lane")   # fk20_fft_plan.hpp: Fk20FftForm
FORM_REPLAY = ("r8", "r8", "r8", "r4", "r2", "r2")                               # the dataflow of each form
HANDOVERS = (8, 16, 48, 128, 512)                                                 # the last n of each form but the last
CLASSES = ("equal", "opposite", "identity")


def form_of(n):
    return sum(n > h for h in HANDOVERS)


def brp7(i):
    return int(format(i, "07b")[::-1], 2)


def bitrev3(v):
    return ((v & 1) << 2) | (v & 2) | ((v >> 2) & 1)


# ---- the reference ----

def _ntt(v, w):
    """out[k] = sum_j v[j] w^(jk), natural order in and out"""
    n = len(v)
    if n == 1:
        return v[:]
    e, o = _ntt(v[0::2], w * w % R), _ntt(v[1::2], w * w % R)
    out, t = [0] * n, 1
    for k in range(n // 2):
        x = t * o[k] % R
        out[k], out[k + n // 2] = (e[k] + x) % R, (e[k] - x) % R
        t = t * w % R
    return out


def expect(a):
    h = _ntt([x % R for x in a], W[127])
    return _ntt(h[:64] + [0] * 64, W[1])


def expect_naive(a):
    h = [sum(a[f] * W[(-f * j) % 128] for f in range(128)) % R for j in range(64)]
    return [sum(h[j] * W[(j * k) % 128] for j in range(64)) % R for k in range(128)]


# ---- additions as events ----

class Events:
    """what every addition of a replay met: count[(site, kind)]; site is a tuple whose first entries name the site class
    (site_class) and whose last ones the stage or the term"""

    def __init__(self, watch=()):
        self.count = Counter()
        # the (full) sites to watch: seen[site] = [(x, y as added)] in the order of the replay
        self.watch, self.seen = watch, {site: [] for site in watch}

    def add(self, site, x, y, neg=False):
        """x + y (x - y with neg) mod r, classified"""
        x, y = x % R, y % R
        if neg:
            y = -y % R
        if x == 0 or y == 0:
            kind = "both" if x == 0 and y == 0 else ("left" if x == 0 else "right")
        elif x == y:
            kind = "equal"
        elif (x + y) % R == 0:
            kind = "opposite"
        else:
            kind = "plain"
        self.count[(site, kind)] += 1
        if site in self.watch:
            self.seen[site].append((x, y))
        return (x + y) % R

    def by_class(self, depth):
        """count[(site[:depth], class)] with left / right / both merged into `identity`"""
        out = Counter()
        for (site, kind), c in self.count.items():
            if kind != "plain":
                out[(site[:depth], kind if kind in ("equal", "opposite") else "identity")] += c
        return out

    def merge(self, other):
        self.count.update(other.count)


def _mulw(v, e):
    return v * W[e % 128] % R


# ---- radix-2 (k_g1_fft_addsub, k_g1_fft_twiddle / _quad, k_g1_fft_fold) ----

def replay_r2(a, ev=None, trace=None):
    ev = ev if ev is not None else Events()
    d = [x % R for x in a]

    def addsub(s, tag):
        half = 1 << (s - 1)
        for bf in range(64):
            j = bf & (half - 1)
            i0 = ((bf >> (s - 1)) << s) + j
            i1 = i0 + half
            u, v = d[i0], d[i1]
            d[i0] = ev.add(("r2", tag, "add", s), u, v)
            d[i1] = ev.add(("r2", tag, "sub", s), u, v, True)

    def twiddle(s, inverse):
        half = 1 << (s - 1)
        for bf in range(64):
            j = bf & (half - 1)
            i1 = ((bf >> (s - 1)) << s) + j + half
            e = j * (128 >> s)
            d[i1] = _mulw(d[i1], -e if inverse else e)

    for s in range(7, 1, -1):
        addsub(s, "dif")
        twiddle(s, True)
        if trace is not None:
            trace.append((("r2", "dif", s), d[:]))
    for g in range(64):
        d[2 * g] = d[2 * g + 1] = ev.add(("r2", "fold"), d[2 * g], d[2 * g + 1])
    if trace is not None:
        trace.append((("r2", "fold"), d[:]))
    for s in range(2, 8):
        twiddle(s, False)
        addsub(s, "dit")
        if trace is not None:
            trace.append((("r2", "dit", s), d[:]))
    return d, ev


# ---- radix-4 (k_g1_fft_r4_ladder, k_g1_fft_r4_post, k_g1_fft_fold) ----

def _r4_group(grp, s, dif):
    if dif:
        q = 1 << (s - 2)
        blk, t = divmod(grp, q)
        p0 = (blk << s) + t
        return t, (p0, p0 + q, p0 + 2 * q, p0 + 3 * q)
    h = 1 << (s - 1)
    blk, t = divmod(grp, h)
    p0 = (blk << (s + 1)) + t
    return t, (p0, p0 + h, p0 + 2 * h, p0 + 3 * h)


def _r4_exponents(t, s, dif):
    e = 128 >> s
    if dif:
        return (t * e, t * e + 32, 3 * t * e, 3 * t * e + 32, 2 * t * e)
    g = t * e // 2
    return (2 * g, g, 3 * g, g + 32, 3 * g + 32)


def replay_r4(a, ev=None, trace=None):
    ev = ev if ev is not None else Events()
    d = [x % R for x in a]
    for s in (7, 5, 3):   # DIF pairs (s, s - 1), inverse twiddles
        out = [0] * 128
        for grp in range(32):
            t, (p0, p1, p2, p3) = _r4_group(grp, s, True)
            a0, a1, a2, a3 = d[p0], d[p1], d[p2], d[p3]
            ex = _r4_exponents(t, s, True)
            v02 = ev.add(("r4", "dif", "lad a0-a2", s), a0, a2, True)       # ladders 0 and 2
            v13 = ev.add(("r4", "dif", "lad a1-a3", s), a1, a3, True)       # ladders 1 and 3
            v4 = ev.add(("r4", "dif", "lad a0+a2", s), a0, a2)              # ladder 4
            c4 = ev.add(("r4", "dif", "lad a1+a3", s), a1, a3)
            v4 = ev.add(("r4", "dif", "lad (a0+a2)-(a1+a3)", s), v4, c4, True)
            lad = [_mulw(v, -e) for v, e in zip((v02, v13, v02, v13, v4), ex)]
            r = ev.add(("r4", "dif", "post a0+a2", s), a0, a2)
            c = ev.add(("r4", "dif", "post a1+a3", s), a1, a3)
            out[p0] = ev.add(("r4", "dif", "post (a0+a2)+(a1+a3)", s), r, c)
            out[p1] = lad[4]
            out[p2] = ev.add(("r4", "dif", "post L0+L1", s), lad[0], lad[1])
            out[p3] = ev.add(("r4", "dif", "post L2-L3", s), lad[2], lad[3], True)
        d = out
        if trace is not None:
            trace.append((("r4", "dif", s), d[:]))
    for g in range(64):
        d[2 * g] = d[2 * g + 1] = ev.add(("r4", "fold"), d[2 * g], d[2 * g + 1])
    if trace is not None:
        trace.append((("r4", "fold"), d[:]))
    for s in (2, 4, 6):   # DIT pairs (s, s + 1)
        out = [0] * 128
        for grp in range(32):
            t, (p0, p1, p2, p3) = _r4_group(grp, s, False)
            x0, x1, x2, x3 = d[p0], d[p1], d[p2], d[p3]
            lad = [_mulw(v, e) for v, e in zip((x1, x2, x3, x2, x3), _r4_exponents(t, s, False))]
            y0 = ev.add(("r4", "dit", "post y0=x0+L0", s), x0, lad[0])
            y1 = ev.add(("r4", "dit", "post y1=x0-L0", s), x0, lad[0], True)
            u = ev.add(("r4", "dit", "post u=L1+L2", s), lad[1], lad[2])
            v = ev.add(("r4", "dit", "post v=L3-L4", s), lad[3], lad[4], True)
            out[p0] = ev.add(("r4", "dit", "post y0+u", s), y0, u)
            out[p1] = ev.add(("r4", "dit", "post y1+v", s), y1, v)
            out[p2] = ev.add(("r4", "dit", "post y0-u", s), y0, u, True)
            out[p3] = ev.add(("r4", "dit", "post y1-v", s), y1, v, True)
        d = out
        if trace is not None:
            trace.append((("r4", "dit", s), d[:]))
    return d, ev


# ---- radix-8 (k_g1_fft_r8_ladder* , k_g1_fft_r8_post, k_g1_fft_fold_raw) ----

R8_RJ = [(4, 0), (2, 0), (2, 1), (6, 0), (6, 1)] + [(r, j) for r in (1, 3, 5, 7) for j in range(4)]   # ladder 0..20 of a group


def _r8_group(grp, s, dif):
    lgn = s if dif else s + 2
    q, e = 1 << (lgn - 3), 128 >> lgn
    blk, t = divmod(grp, q)
    return t, blk << lgn, q, e


def _vname(r):
    return "V(4,0)" if r == 4 else ("V(2|6,j)" if r in (2, 6) else "V(odd,j)")


def replay_r8(a, ev=None, trace=None):
    ev = ev if ev is not None else Events()
    d = [x % R for x in a]
    for s in (7, 4):   # DIF triples (s, s - 1, s - 2), inverse twiddles
        out = [0] * 128
        for grp in range(16):
            t, base, q, e = _r8_group(grp, s, True)
            x = [d[base + t + q * m] for m in range(8)]
            lad = {}
            for r, j in R8_RJ:
                step = 1 if r == 4 else (4 if r & 1 else 2)
                v = x[j]
                for k in range(1, 8 // step):   # first term x_j, then alternating signs
                    v = ev.add(("r8", "dif", _vname(r), k, s), v, x[j + step * k], k & 1 == 1)
                lad[(r, j)] = _mulw(v, -(e * r * t + 16 * r * j))
            for c in range(8):
                r = bitrev3(c)
                if r == 0:
                    acc = x[0]
                    for m in range(1, 8):
                        acc = ev.add(("r8", "dif", "post r=0", m, s), acc, x[m])
                else:
                    acc = lad[(r, 0)]
                    for j in range(1, 1 if r == 4 else (4 if r & 1 else 2)):
                        acc = ev.add(("r8", "dif", "post r=2|6" if r in (2, 6) else "post r odd", j, s), acc, lad[(r, j)])
                out[base + c * q + t] = acc
        d = out
        if trace is not None:
            trace.append((("r8", "dif", s), d[:]))
    for g in range(64):
        d[2 * g] = d[2 * g + 1] = ev.add(("r8", "fold"), d[2 * g], d[2 * g + 1])
    if trace is not None:
        trace.append((("r8", "fold"), d[:]))
    for s in (2, 5):   # DIT triples (s, s + 1, s + 2)
        out = [0] * 128
        for grp in range(16):
            t, base, q, e = _r8_group(grp, s, False)
            y = [d[base + bitrev3(r) * q + t] for r in range(8)]
            lad = {(r, j): _mulw(y[r], e * r * t + 16 * r * j) for r, j in R8_RJ}
            for m in range(8):
                acc = y[0]
                terms = [((4, 0), m & 1), ((2, m & 1), (m >> 1) & 1), ((6, m & 1), (m >> 1) & 1)]
                terms += [((r, m & 3), (m >> 2) & 1) for r in (1, 3, 5, 7)]
                for k, (rj, neg) in enumerate(terms):
                    acc = ev.add(("r8", "dit", "post", k, s), acc, lad[rj], neg == 1)
                out[base + t + q * m] = acc
        d = out
        if trace is not None:
            trace.append((("r8", "dit", s), d[:]))
    return d, ev


REPLAYS = {"r2": replay_r2, "r4": replay_r4, "r8": replay_r8}
# How many leading entries of a site name its class.  CLASS_DEPTH: the site classes of the coverage condition --
# radix-2 addsub per stage and the fold, each radix-4 site, each V, each post sum and the fold of radix-8.
# FINE_DEPTH: the whole site, down to the step and the term of a multi-term sum (the second, stricter condition).
CLASS_DEPTH = {"r2": 4, "r4": 3, "r8": 3}
FINE_DEPTH = 9


def sites(kind, depth):
    """every site of a dataflow at that depth: those a generic vector visits (every addition is performed whatever
    the operands are)"""
    ev = Events()
    REPLAYS[kind]([random.Random(5).randrange(1, R) for _ in range(128)], ev)
    return sorted({site[:depth] for site, _ in ev.count}, key=str)


def coverage(kind, vectors, depth=None):
    """(Events over all vectors, Counter by (site[:depth], class))"""
    ev = Events()
    for _, a in vectors:
        REPLAYS[kind](a, ev)
    return ev, ev.by_class(CLASS_DEPTH[kind] if depth is None else depth)


def missing(kind, vectors, depth):
    _, cov = coverage(kind, vectors, depth)
    return [(site, cls) for site in sites(kind, depth) for cls in CLASSES if cov[(site, cls)] == 0]


# ---- the corpus ----

A = random.Random(0xF20).randrange(1, R)
TONES = (0, 1, 2, 16, 32, 63, 64, 65, 96, 127)
DELTAS = (0, 1, 64, 127)
SMALL_SEEDS = 8


def named_vectors():
    """the vectors built from one scalar a = A (random, not zero): [(name, 128 scalars)]"""
    rnd = random.Random(20)
    out = [("random", [rnd.randrange(1, R) for _ in range(128)]), ("const", [A] * 128)]
    out += [("delta_%d" % f, [A if g == f else 0 for g in range(128)]) for f in DELTAS]
    out += [("tone_%d" % m, [A * W[(f * m) % 128] % R for f in range(128)]) for m in TONES]
    out += [("halves", [A if f < 64 else -A % R for f in range(128)]), ("zero", [0] * 128)]
    # the shape of the FK20 input of the blob a x^64 + r(x), deg r < 64: generic points whose inverse transform is a at
    # j = 0, the identity at j = 1..63 and generic above (which the truncation drops) -- 63 of the 64 fold additions
    # cancel on operands that share nothing but their sum, and every output is 128 a
    hi = [0] * 64 + [rnd.randrange(1, R) for _ in range(64)]
    out.append(("fold_cancel", [(A + x) % R for x in _ntt(hi, W[1])]))
    for seed in range(SMALL_SEEDS):
        r2 = random.Random(1000 + seed)
        out.append(("small_%d" % seed, [r2.choice((0, A, -A, 2 * A, -2 * A)) % R for _ in range(128)]))
    return out


def solve_sites(kind, wanted, seed, shift=0):
    """a generic vector with len(wanted) of its entries solved so that addition number shift + i (mod the number of
    times the site occurs) of site wanted[i][0] meets wanted[i][1] (`equal`: x = y, `opposite`: x = -y): every operand
    of every addition is linear in the inputs, so the conditions are a linear system (g1_expect.solve_affine does the
    same for the sum stages, one replay per constraint; here one replay gives all of them).  Conditions that contradict
    each other -- two in one accumulation chain -- give a singular system (None) or a vector that misses some."""
    rnd = random.Random(seed)
    a = [rnd.randrange(1, R) for _ in range(128)]
    n = len(wanted)
    free = rnd.sample(range(128), n)
    watch = {site for site, _ in wanted}

    def conditions(vec):
        ev = Events(watch=watch)
        REPLAYS[kind](vec, ev)
        out = []
        for i, (site, cls) in enumerate(wanted):
            x, y = ev.seen[site][(shift + i) % len(ev.seen[site])]
            out.append((x - y if cls == "equal" else x + y) % R)
        return out

    for j in free:
        a[j] = 0
    f0 = conditions(a)
    m = [[0] * (n + 1) for _ in range(n)]
    for col, j in enumerate(free):
        a[j] = 1
        for row, v in enumerate(conditions(a)):
            m[row][col] = (v - f0[row]) % R
        a[j] = 0
    for row in range(n):
        m[row][n] = -f0[row] % R
    for col in range(n):
        piv = next((r_ for r_ in range(col, n) if m[r_][col]), None)
        if piv is None:
            return None
        m[col], m[piv] = m[piv], m[col]
        inv = pow(m[col][col], -1, R)
        m[col] = [v * inv % R for v in m[col]]
        for r_ in range(n):
            if r_ != col and m[r_][col]:
                f = m[r_][col]
                m[r_] = [(v - f * w) % R for v, w in zip(m[r_], m[col])]
    for col, j in enumerate(free):
        a[j] = m[col][n]
    return a


_CORPUS = None


def corpus():
    """[(name, 128 scalars)]: the named vectors, then for each dataflow the vectors solved for the doublings and the
    cancellations the named ones do not reach at some step or term (FINE_DEPTH): y1 and v of a radix-4 DIT pair, the
    running sum of a radix-8 post sum against its third term -- operands that come from ladders with different
    twiddles and so never coincide on multiples of one scalar"""
    global _CORPUS
    if _CORPUS is None:
        out = named_vectors()
        for kind in ("r2", "r4", "r8"):
            for rnd_no in range(6):
                want = [(s, c) for s, c in missing(kind, out, FINE_DEPTH) if c != "identity"]
                if not want:
                    break
                vec = solve_sites(kind, want, seed=100 * rnd_no + len(want), shift=5 * rnd_no)
                if vec is not None:
                    out.append(("solved_%s_%d" % (kind, rnd_no), vec))
        _CORPUS = out
    return _CORPUS
