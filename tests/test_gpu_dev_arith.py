"""The arithmetic only the GPU runs -- the F28 product as the device compiler builds it, its inline-asm form
(CKZG_F28_ASM_BLOCKS: what msm.hip and fk20.hip run), all of g1_quad.hpp and the straight-line routines of
g1_pipe.hpp (xyzz28_addsub_quad, jac28_add_quad_pipe, naf2_128, naf_masks), f28_inv_safegcd in both forms and g1.hpp's
complete xyzz_add / xyzz_dbl on 32-bit limbs (what k_point_lhs sums its ladder results with) -- fed chosen inputs through tests/native/dev_shim.hip (libdev_shim.so: one source, two builds,
ds_plain_* / ds_asm_*) and compared with exact references: Python integers for the field (tests/arith_cases.py,
no tolerance: the product must equal (a b + q p) >> 392 limb for limb), the CPU oracle for the group law.

Geometry.  Field lists run twice: whole, in workgroups of 256, and their first 101 items (every input class is
among them) in workgroups of 64, which leaves a wave with 37 live lanes.  Point kernels give every item a DPP quad
and return the result of EACH of the four lanes; the lanes must agree byte for byte.  The item counts (61, 49,
25, 13, ...) leave the last wave with only some of its 16 quads holding real items.  Partly filled QUADS are never
launched, because the product never launches them: its quad kernels pad a wave's idle quads with a repeat of the
last item and mask only the store (fk20.hip k_g1_fft_twiddle_quad, verify.hip k_subgroup_g1_quad), and the shim
pads the same way -- a DPP read of an inactive lane would return 0.

After any non-zero return of a shim call (a HIP error or the shim's 20 s deadline) every later test of the module
fails at once without launching anything.

The exceptional-case fallbacks of the quad additions (equal or opposite operands) are reached directly
(test_additions), by the w4_128 quad ladder while it builds its table (P + P) and on the points outside the subgroup
of test_subgroup_and_bls_x.  Inside a ladder over a point of the prime-order subgroup they cannot be: the partial
sums of a scalar below r never meet a table entry.  The small scalars 2, 3, 6, 14 are run nevertheless."""
import ctypes as C
import os
import random
import subprocess

import pytest

import arith_cases as ac
from arith_cases import LAMBDA, P, R
from conftest import ORACLE_SO, ROOT, SHIM_SO

pytestmark = pytest.mark.gpu

# CKZG_DEV_SHIM_SO: another build of the shim (the way conftest.py takes CKZG_HIP_SO / CKZG_SHIM_SO)
DEV_SHIM_SO = os.path.abspath(os.environ["CKZG_DEV_SHIM_SO"]) if os.environ.get("CKZG_DEV_SHIM_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "libdev_shim.so")
FORMS = ["plain", "asm"]
# every exported function this module binds, once per form (tests/test_dev_shim_cpu.py checks the library for them)
SHIM_FUNCTIONS = ["f28_ops", "field", "f28_inv", "g1_add", "g1_dbl", "g1_mul", "g1_subgroup", "g1_chain", "g1_eat", "g1_reduce", "naf"]
# the one plain build of tests/native/dev_shim_fields.hip in the same library (tests/test_gpu_fields.py)
DEV_FUNCTIONS = ["ds_dev_field_ops", "ds_dev_field"]
ONE = (pow(2, 384, P)).to_bytes(48, "little")
INF = bytes(144)
BLS_X = 0xd201000000010000


class DevShim:
    """libdev_shim.so; remembers the first failed call and refuses every later one"""

    def __init__(self, lib):
        self.lib = lib
        self.dead = None

    def call(self, form, name, *args):
        if self.dead is not None:
            pytest.fail("an earlier shim call (%s) returned %d: nothing is launched any more" % self.dead)
        rc = getattr(self.lib, "ds_%s_%s" % (form, name))(*args)
        if rc != 0:
            self.dead = ("ds_%s_%s" % (form, name), rc)
            pytest.fail("ds_%s_%s returned %d" % (form, name, rc))


class Group:
    """points as 144-byte Jacobian strings, arithmetic by the CPU oracle"""

    def __init__(self, o, h):
        self.o = o
        g = C.create_string_buffer(144)
        h.hs_g1_generator(g)
        self.g = g.raw

    def _b(self, raw=None):
        b = C.create_string_buffer(144)
        if raw is not None:
            b.raw = raw
        return b

    def mul(self, p, k):
        r = self._b()
        self.o.og1_mul_raw(r, self._b(p), (C.c_uint64 * 4)(*[(k >> (64 * i)) & (2 ** 64 - 1) for i in range(4)]), 255)
        return r.raw

    def add(self, a, b):
        r = self._b()
        self.o.og1_add(r, self._b(a), self._b(b))
        return r.raw

    def dbl(self, a):
        r = self._b()
        self.o.og1_dbl(r, self._b(a))
        return r.raw

    def neg(self, a):
        r = self._b()
        self.o.og1_neg(r, self._b(a))
        return r.raw

    def is_inf(self, a):
        return bool(self.o.og1_is_inf(self._b(a)))

    def equal(self, a, b):
        return bool(self.o.og1_equal(self._b(a), self._b(b)))

    def in_subgroup(self, a):
        return bool(self.o.og1_in_subgroup(self._b(a)))

    def affine(self, p):
        """the same point with Z = 1 (infinity stays all zero)"""
        if self.is_inf(p):
            return INF
        a = C.create_string_buffer(96)
        self.o.og1_to_affine(a, self._b(p))
        return a.raw + ONE

    def rand(self, rnd):
        return self.mul(self.g, rnd.randrange(1, R))

    def curve_point(self, x0):
        x, y = ac.curve_point_xy(x0)
        r384 = pow(2, 384, P)
        return (x * r384 % P).to_bytes(48, "little") + (y * r384 % P).to_bytes(48, "little") + ONE


@pytest.fixture(scope="module")
def env():
    pkg = os.path.join(ROOT, "c-kzg-4844_amd")
    if not os.path.exists(DEV_SHIM_SO):
        subprocess.check_call(["make", "-C", pkg, "-j", "2", "libdev_shim.so"])
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", pkg, "csrc/libhost_shim.so"])
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    o, h, d = C.CDLL(ORACLE_SO), C.CDLL(SHIM_SO), C.CDLL(DEV_SHIM_SO)
    for fn in ("og1_equal", "og1_is_inf", "og1_in_subgroup"):
        getattr(o, fn).restype = C.c_bool
    for form in FORMS:
        getattr(d, "ds_%s_f28_ops" % form).restype = C.c_char_p
    return Group(o, h), DevShim(d)


def _lanes(grp, out, i, stride=144, per_lane=1):
    """the four lanes' results of item i; asserts that they are identical"""
    size = stride * per_lane
    lanes = [out[(4 * i + l) * size:(4 * i + l + 1) * size] for l in range(4)]
    assert lanes[0] == lanes[1] == lanes[2] == lanes[3], ("lanes of item %d differ" % i)
    return lanes[0]


def _words8(k):
    return [(k >> (32 * i)) & 0xffffffff for i in range(8)]


# ---- field ----

def _field_kinds():
    return sorted(ac.REQUIRED_KINDS)


@pytest.mark.parametrize("kind", _field_kinds())
@pytest.mark.parametrize("form", FORMS)
def test_field_corpora(env, form, kind):
    _, shim = env
    ops = ac.parse_ops(getattr(shim.lib, "ds_%s_f28_ops" % form)().decode())
    for want in ac.REQUIRED_OPS:
        assert want in ops, want
    assert {name for name, _ in ops} == ac.REQUIRED_KINDS
    ran = 0
    for k, op in enumerate(ops):
        if op[0] != kind:
            continue
        cases, _, _ = ac.field_reference(op)
        a, b, c, d = ac.pack_operands(cases)
        for count, block in ((len(cases), 256), (ac.SUBSET_LEN, 64)):
            out = (C.c_uint32 * (14 * len(cases)))()
            shim.call(form, "field", k, out, a, b, c, d, count, block)
            ac.check_field_run(op, out, count)
        ran += 1
    assert ran


@pytest.mark.parametrize("form", FORMS)
def test_f28_inv_safegcd(env, form):
    """f28_inv_safegcd ends in an F28 product, so it exists in both forms: the inputs of tests/field_cases.py (chosen as
    the integer that reaches the divsteps, lanes of a wave leaving the loop after different numbers of batches)"""
    import field_cases as fc
    _, shim = env
    items, wants = fc.cached_corpus("f28_inv_safegcd")
    a = (C.c_uint32 * (14 * len(items)))(*[w for it in items for w in it[0]])
    for count, block in ((len(items), 256), (fc.SUBSET_LEN, 64)):
        out = (C.c_uint32 * (14 * len(items)))()
        shim.call(form, "f28_inv", out, a, count, block)
        fc.check("f28_inv_safegcd", wants, out, 14, count)


# ---- additions ----

ADD_KINDS = {0: "xyzz28_add", 1: "jac28_add", 2: "xyzz28_madd", 3: "jac28_add_quad", 4: "jac28_add_quad_zz",
             5: "jac28_madd_quad_zz", 6: "jac28_add_quad_pipe", 7: "xyzz28_add_quad", 8: "xyzz28_addsub_quad",
             9: "xyzz_add"}               # g1.hpp's complete addition on 32-bit limbs: k_point_lhs sums its ladder results with it


@pytest.fixture(scope="module")
def add_cases(env):
    """(a, b, negate b) with the oracle's a + (+-b): generic, P + P (the fallback must double), P + (-P) (infinity),
    accumulator at infinity, b at infinity, both signs of each, P + phi(P) and 2P + P (no shared coordinate, small
    h), padded with generic pairs"""
    grp, _ = env
    rnd = random.Random(4001)
    cases = []
    for _ in range(3):
        p, q = grp.rand(rnd), grp.rand(rnd)
        pairs = [(p, q), (p, p), (p, grp.neg(p)), (INF, q), (p, INF), (INF, INF), (p, grp.mul(p, LAMBDA)),
                 (grp.dbl(p), p), (grp.affine(p), grp.affine(p)), (grp.affine(p), q)]
        cases += [(a, b, neg) for a, b in pairs for neg in (0, 1)]
    while len(cases) < 61:             # 61 quads (49 without the b-at-infinity cases): the last wave is part padding
        cases.append((grp.rand(rnd), grp.rand(rnd), rnd.randrange(2)))
    return [(a, b, neg, grp.add(a, grp.neg(b) if neg else b)) for a, b, neg in cases]


@pytest.mark.parametrize("kind", sorted(ADD_KINDS), ids=lambda k: ADD_KINDS[k])
@pytest.mark.parametrize("form", FORMS)
def test_additions(env, add_cases, form, kind):
    grp, shim = env
    cases = add_cases
    if kind not in (0, 7, 8, 9):       # only the XYZZ forms take a second operand at infinity
        cases = [c for c in cases if c[1] != INF]
    assert len(cases) >= 37 and len(cases) % 16 != 0
    affine_b = kind in (2, 5)          # the mixed additions take an affine point
    n = len(cases)
    a = b"".join(c[0] for c in cases)
    b = b"".join(grp.affine(c[1]) if affine_b else c[1] for c in cases)
    flags = bytes(c[2] for c in cases)
    out, zzok = C.create_string_buffer(4 * n * 144), C.create_string_buffer(4 * n)
    shim.call(form, "g1_add", kind, out, zzok, a, b, flags, n, 64)
    for i, (pa, pb, neg, want) in enumerate(cases):
        got = _lanes(grp, out.raw, i)
        assert grp.equal(got, want), (ADD_KINDS[kind], i, neg)
        assert zzok.raw[4 * i:4 * i + 4] == b"\x01" * 4, (ADD_KINDS[kind], i, "carried Z^2")


# ---- doublings ----

DBL_KINDS = {0: "jac28_dbl", 1: "jac28_dbl_quad", 2: "jac28_dbl_quad_zz", 3: "xyzz_dbl"}     # 3: g1.hpp, 32-bit limbs


@pytest.fixture(scope="module")
def dbl_cases(env):
    grp, _ = env
    rnd = random.Random(4002)
    cases = []
    for t in range(2):
        p = grp.rand(rnd)
        for n in [0] + ac.DBL_CHAIN_LENGTHS:
            want = p
            for _ in range(n):
                want = grp.dbl(want)
            cases.append((p if t else grp.affine(p), n, want))
    return cases[:13]


@pytest.mark.parametrize("kind", sorted(DBL_KINDS), ids=lambda k: DBL_KINDS[k])
@pytest.mark.parametrize("form", FORMS)
def test_doubling_chains(env, dbl_cases, form, kind):
    grp, shim = env
    n = len(dbl_cases)
    assert {c[1] for c in dbl_cases} >= set(ac.DBL_CHAIN_LENGTHS)
    a = b"".join(c[0] for c in dbl_cases)
    steps = (C.c_uint32 * n)(*[c[1] for c in dbl_cases])
    out, zzok = C.create_string_buffer(4 * n * 144), C.create_string_buffer(4 * n)
    shim.call(form, "g1_dbl", kind, out, zzok, a, steps, n, 64)
    for i, (_, ns, want) in enumerate(dbl_cases):
        assert grp.equal(_lanes(grp, out.raw, i), want), (DBL_KINDS[kind], ns)
        assert zzok.raw[4 * i:4 * i + 4] == b"\x01" * 4, (DBL_KINDS[kind], ns, "zz == Z^2 after every doubling")


# ---- scalar multiplications ----

MUL_KINDS = {0: "xyzz28_mul_w4", 1: "xyzz28_mul_glv_w4", 2: "xyzz28_mul_glv_naf", 3: "xyzz28_mul_w4_128",
             4: "xyzz28_mul_w4_128_quad", 5: "xyzz28_mul_glv_naf_quad"}


@pytest.fixture(scope="module")
def mul_cases(env):
    """per kind: [(point, 8 scalar words, halves?, expected)]"""
    grp, _ = env
    rnd = random.Random(4003)
    p1 = grp.rand(rnd)
    full = ac.glv_scalars(random.Random(29))
    order3 = grp.curve_point(0)
    assert not grp.is_inf(order3) and grp.is_inf(grp.mul(order3, 3))
    halves = ac.HALF_SCALARS + ac.SELF_MEETING_SCALARS + [k % LAMBDA for k in full] + [k // LAMBDA for k in full]
    halves += [rnd.randrange(1 << 128) for _ in range(40)]      # with both halves of every lambda-adjacent scalar and twiddle power
    out = {}
    # the 255-bit window ladder: the scalar lists of test_xyzz28_full_add_mul_neg, the order-3 point, infinity in
    c0 = [(p1, k) for k in ac.W4_SCALARS + full[:30]] + [(order3, k) for k in ac.ORDER3_SCALARS] + [(INF, full[20])]
    out[0] = [(p, _words8(k), 0, grp.mul(p, k)) for p, k in c0]
    # the GLV ladders: every scalar of test_glv_split_and_glv_scalar_mul (lambda-adjacent, twiddle powers, random)
    cg = [(p1, k) for k in full] + [(INF, full[20])] + [(p1, k) for k in ac.SELF_MEETING_SCALARS]
    glv = [(p, _words8(k), 0, grp.mul(p, k)) for p, k in cg]
    pairs = [(a, b) for a in ac.HALF_SCALARS for b in ac.HALF_SCALARS] + [(k, 0) for k in ac.SELF_MEETING_SCALARS] + \
            [(0, k) for k in ac.SELF_MEETING_SCALARS] + [(k, k) for k in ac.SELF_MEETING_SCALARS] + [(5, 7)]
    glv_h = [(p1, _words8(a | (b << 128)), 1, grp.mul(p1, (a + LAMBDA * b) % R)) for a, b in pairs]
    out[1] = glv
    out[2] = out[5] = glv + glv_h
    # one 128-bit half
    ch = [(p1, k) for k in halves] + [(INF, 5)]
    out[3] = out[4] = [(p, _words8(k), 0, grp.mul(p, k)) for p, k in ch]
    return out


@pytest.mark.parametrize("kind", sorted(MUL_KINDS), ids=lambda k: MUL_KINDS[k])
@pytest.mark.parametrize("form", FORMS)
def test_scalar_multiplications(env, mul_cases, form, kind):
    grp, shim = env
    for halves in (0, 1):
        cases = [c for c in mul_cases[kind] if c[2] == halves]
        if not cases:
            continue
        n = len(cases)
        assert n % 16 != 0             # the last wave holds padding quads
        pts = b"".join(c[0] for c in cases)
        ks = (C.c_uint32 * (8 * n))(*[w for c in cases for w in c[1]])
        out = C.create_string_buffer(4 * n * 144)
        shim.call(form, "g1_mul", kind, out, pts, ks, halves, n, 64)
        for i, c in enumerate(cases):
            assert grp.equal(_lanes(grp, out.raw, i), c[3]), (MUL_KINDS[kind], halves, i, c[1])


# ---- the digit recoding of the pipelined ladders ----

@pytest.mark.parametrize("form", FORMS)
def test_naf_recoding(env, form):
    """naf2_128 as the device compiler builds it and naf_masks on its output (item i as chain 0, item i + 1 as
    chain 1): the digits are the non-adjacent form of k, the nz / neg words spell those digits and `top` is the
    highest bit with a non-zero digit in either chain.  One thread per item: a whole workgroup of 256 and a last
    wave with 47 live lanes"""
    _, shim = env
    ks = ac.naf_scalars()
    n = len(ks)
    assert n > 64 and n % 64 != 0
    words = (C.c_uint32 * (4 * n))(*[(k >> (32 * j)) & 0xffffffff for k in ks for j in range(4)])
    for block in (256, 64):
        digits, masks = (C.c_int8 * (ac.NAF2_LEN * n))(), (C.c_uint64 * (13 * n))()
        shim.call(form, "naf", digits, masks, words, n, block)
        ds = [digits[ac.NAF2_LEN * i:ac.NAF2_LEN * (i + 1)] for i in range(n)]
        for i, k in enumerate(ks):
            ac.check_naf2(k, ds[i])
            want = ac.naf_masks_expected(ds[i], ds[(i + 1) % n])
            got = list(masks[13 * i:13 * i + 12]) + [masks[13 * i + 12] - (1 << 64) * (masks[13 * i + 12] >> 63)]
            assert got == want, (k, ks[(i + 1) % n], got, want)


# ---- subgroup test ----

SUBGROUP_KINDS = {0: "g1_28_in_subgroup", 1: "g1_28_in_subgroup_quad", 2: "jac28_mul_bls_x_quad", 3: "jac28_mul_bls_x"}


@pytest.fixture(scope="module")
def subgroup_cases(env):
    """the corpus of test_endomorphism_subgroup_test_is_exact: G1 points, (0, 2) of order 3, random curve points,
    their [r]P (cofactor torsion), mixed points; with the oracle's [r]P == infinity and [|x|]P"""
    grp, _ = env
    rnd = random.Random(31)
    pts = [grp.rand(rnd) for _ in range(6)] + [grp.curve_point(0)]
    for _ in range(6):
        pt = grp.curve_point(rnd.randrange(P))
        tors = grp.mul(pt, R)
        assert not grp.is_inf(tors)
        pts += [pt, tors, grp.add(tors, grp.rand(rnd))]
    cases = [(grp.affine(p), grp.in_subgroup(p), grp.mul(p, BLS_X)) for p in pts]
    assert [c[1] for c in cases] == [True] * 6 + [False] * 19
    return cases


@pytest.mark.parametrize("kind", sorted(SUBGROUP_KINDS), ids=lambda k: SUBGROUP_KINDS[k])
@pytest.mark.parametrize("form", FORMS)
def test_subgroup_and_bls_x(env, subgroup_cases, form, kind):
    grp, shim = env
    n = len(subgroup_cases)
    pts = b"".join(c[0] for c in subgroup_cases)
    out, verdict = C.create_string_buffer(4 * n * 144), C.create_string_buffer(4 * n)
    shim.call(form, "g1_subgroup", kind, out, verdict, pts, n, 64)
    for i, (_, member, xp) in enumerate(subgroup_cases):
        if kind < 2:
            assert verdict.raw[4 * i:4 * i + 4] == (b"\x01" if member else b"\x00") * 4, (SUBGROUP_KINDS[kind], i)
        else:
            assert grp.equal(_lanes(grp, out.raw, i), xp), (SUBGROUP_KINDS[kind], i)


# ---- chains of mixed additions ----

@pytest.fixture(scope="module")
def chain_cases(env):
    """[(points, signs, expected)]: the alternation scripts of test_xyzz28_sign_alternating_accumulation and the
    200-point chain of test_xyzz28_mixed_addition_matches_oracle"""
    grp, _ = env
    rnd = random.Random(23)
    base = [grp.rand(rnd) for _ in range(12)]
    chains = []
    for sc in ac.alternation_scripts(rnd):
        special = None
        if isinstance(sc, tuple):
            special, sc = sc
        pts, signs, ref = [grp.affine(base[i]) for i, _ in sc], [s for _, s in sc], INF
        for i, sgn in sc:
            ref = grp.add(ref, grp.neg(base[i]) if sgn else base[i])
        if special == "dbl":
            pts.append(grp.affine(ref))
            signs.append(0)
            ref = grp.dbl(ref)
        chains.append((pts, signs, ref))
    pts, signs, ref = [], [], INF
    for i in range(200):
        p = grp.rand(rnd)
        pts.append(grp.affine(p))
        signs.append(i & 1)
        ref = grp.add(ref, grp.neg(p) if i & 1 else p)
    chains.append((pts, signs, ref))
    return chains


@pytest.mark.parametrize("kind", [0, 1], ids=["xyzz28_madd", "xyzz28_madd_alt"])
@pytest.mark.parametrize("form", FORMS)
def test_mixed_addition_chains(env, chain_cases, form, kind):
    grp, shim = env
    n = len(chain_cases)
    pts = b"".join(p for c in chain_cases for p in c[0])
    signs = bytes(s for c in chain_cases for s in c[1])
    start = [0]
    for c in chain_cases:
        start.append(start[-1] + len(c[0]))
    assert max(len(c[0]) for c in chain_cases) == 200
    out = C.create_string_buffer(n * 144)
    shim.call(form, "g1_chain", kind, out, pts, signs, (C.c_uint32 * (n + 1))(*start), n, 64)
    for i, c in enumerate(chain_cases):
        assert grp.equal(out.raw[144 * i:144 * i + 144], c[2]), (kind, i, len(c[0]))


# ---- the co-Z table ----

@pytest.mark.parametrize("form", FORMS)
def test_coz_table_quad(env, form):
    """eat28_build_quad (coz28_addu_quad inside): the table mapped home equals {P, 3P, 5P, 7P} and its phi images,
    by the oracle and by eat28_build on the same point"""
    grp, shim = env
    rnd = random.Random(77)
    pts = [grp.rand(rnd) for _ in range(5)]
    pts = pts + [grp.affine(pts[0])]
    n = len(pts)
    out = C.create_string_buffer(64 * n * 144)
    shim.call(form, "g1_eat", out, b"".join(pts), n, 64)
    for i, p in enumerate(pts):
        rec = _lanes(grp, out.raw, i, per_lane=16)
        got = [rec[144 * e:144 * e + 144] for e in range(16)]
        for m in range(4):
            want, phi = grp.mul(p, 2 * m + 1), grp.mul(p, (2 * m + 1) * LAMBDA % R)
            assert grp.equal(got[m], want) and grp.equal(got[8 + m], want), (i, m)
            assert grp.equal(got[4 + m], phi) and grp.equal(got[12 + m], phi), (i, m, "phi")


# ---- workgroup folds ----

REDUCE_FORMS = [(64, 1), (256, 1), (64, 0)]    # (threads, quad form): what msm.hip / pippenger.hip / verify.hip instantiate


def _reduce_patterns(grp, T, rnd):
    p, q = grp.rand(rnd), grp.rand(rnd)
    np_ = grp.neg(p)
    pats = [[INF] * T]
    for pos in sorted({0, 1, 63, 64, T - 1}):
        if pos < T:
            pats.append([p if i == pos else INF for i in range(T)])
    pats.append([p] * T)                                             # every pair at every level doubles: [T]P
    pats.append([p if i % 2 == 0 else np_ for i in range(T)])        # neighbours opposite
    pats.append([p if i < T // 2 else np_ for i in range(T)])        # halves opposite
    some = [grp.rand(rnd) for _ in range(8)]
    half = [some[i % 8] if i % 3 else grp.mul(some[i % 8], i + 2) for i in range(T // 2)]
    pats.append(half + [grp.neg(x) for x in reversed(half)])         # sums to infinity, lane i against lane T-1-i
    pats.append([q] * (T // 2) + [grp.neg(q)] * (T // 2 - 1) + [p])  # all but one term cancel
    pats.append([INF if rnd.random() < 0.1 else grp.mul(some[i % 8], rnd.randrange(1, 1 << 20)) for i in range(T)])
    return pats


@pytest.fixture(scope="module")
def reduce_cases(env):
    grp, _ = env
    out = {}
    for T, quad_form in REDUCE_FORMS:
        if T in out:
            continue
        pats = _reduce_patterns(grp, T, random.Random(4004 + T))
        wants = []
        for lanes in pats:
            acc = INF
            for x in lanes:
                acc = grp.add(acc, x)
            wants.append(acc)
        same = [i for i, lanes in enumerate(pats) if lanes[0] != INF and all(x == lanes[0] for x in lanes)]
        assert grp.is_inf(wants[0]) and len(same) == 1 and grp.equal(wants[same[0]], grp.mul(pats[same[0]][0], T))
        out[T] = (pats, wants)
    return out


@pytest.mark.parametrize("threads,quad_form", REDUCE_FORMS, ids=["quad64", "quad256", "lane64"])
@pytest.mark.parametrize("form", FORMS)
def test_workgroup_folds(env, reduce_cases, form, threads, quad_form):
    grp, shim = env
    pats, wants = reduce_cases[threads]
    groups = len(pats)
    out = C.create_string_buffer(groups * 144)
    shim.call(form, "g1_reduce", out, b"".join(x for lanes in pats for x in lanes), groups, threads, quad_form)
    for gidx, want in enumerate(wants):
        assert grp.equal(out.raw[144 * gidx:144 * gidx + 144], want), (threads, quad_form, gidx)
