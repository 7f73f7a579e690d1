"""Fp on 13 signed 30-bit limbs (c-kzg-4844_amd/csrc/fp30.hpp) and the accumulate loop's mixed addition on it
(g1_30.hpp), compiled for the host into libhost_shim.so: limb-exact against Python integers, and the addition chain --
through entry, phi and exit -- against the 28-bit law it replaces in the throughput kernel.  The models and the corpora
are those of tests/fp30_expect.py, shared with the device tests (tests/test_gpu_fp30.py): the whole op list of
f30_test_ops.hpp runs here through hs_f30_run, the addition, phi and the exit on raw state through hs_madd30_step /
hs_phi30 / hs_exit30, and the step model is anchored to the oracle's group law."""
import ctypes as C
import os
import random
import subprocess

import pytest

from arith_cases import P, R
from conftest import ORACLE_SO, ROOT, SHIM_SO

import fp30_expect as fx
from fp30_expect import (HALF, N, W, column_product, extreme_operands, model_product, out_limbs, rand_operand,  # noqa: F401
                         value)

I32x13 = C.c_int32 * N


@pytest.fixture(scope="module")
def libs():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    o, h = C.CDLL(ORACLE_SO), C.CDLL(SHIM_SO)
    o.og1_equal.restype = C.c_bool
    o.og1_is_inf.restype = C.c_bool
    return o, h


def call(h, name, *ops):
    r = I32x13()
    getattr(h, name)(r, *[I32x13(*x) for x in ops])
    return list(r)


def test_constants(libs):
    _, h = libs
    p, r392, r394, beta = I32x13(), I32x13(), I32x13(), I32x13()
    ninv = C.c_uint32()
    h.hs_fp30_consts(p, C.byref(ninv), r392, r394, beta)
    assert value(p) == P and all(abs(v) <= HALF for v in p)
    assert (ninv.value * P) % (1 << W) == (1 << W) - 1
    assert value(r392) == pow(2, 392, P) and value(r394) == pow(2, 394, P)
    b = value(beta) * pow(2, -390, P) % P
    assert b != 1 and pow(b, 3, P) == 1            # a primitive cube root of unity: beta
    # it is the beta of the 28-bit loop (the oracle has no such export; phi is pinned again by the chain test)
    for arr in (r392, r394, beta):
        assert all(abs(v) <= HALF for v in arr)


def test_model_is_the_column_walk():
    rnd = random.Random(30)
    for _ in range(40):
        a, b, c, d = (rand_operand(rnd, v) for v in (17, 17, 5, 5))
        assert column_product(a, b) == model_product(value(a) * value(b))
        assert column_product(a, b, c, d) == model_product(value(a) * value(b) + value(c) * value(d))
    # every limb at the bound, all signs aligned: the fullest columns the static_asserts admit
    for s in (1, -1):
        full = [HALF] * 12 + [0]
        neg = [s * v for v in full]
        column_product(full, neg)
        column_product(full, neg, full, neg)


def test_mul_sqr_mul_add2_norm_exact(libs):
    _, h = libs
    rnd = random.Random(31)
    e17, e18, e5 = extreme_operands(17), extreme_operands(18), extreme_operands(5)
    for k in range(10000 + len(e17) * len(e18)):
        if k < len(e17) * len(e18):
            a, b = e17[k % len(e17)], e18[k // len(e17)]
            b2 = e17[(k // len(e17)) % len(e17)]
            c, d = e5[k % len(e5)], e5[(k // 3) % len(e5)]
        else:
            a, b, b2, c, d = (rand_operand(rnd, v) for v in (17, 18, 17, 5, 5))
        got = call(h, "hs_fp30_mul", a, b)
        assert got == model_product(value(a) * value(b)), (a, b)
        assert abs(value(got)) <= P and all(abs(v) <= HALF for v in got)
        assert (value(got) << 390) % P == value(a) * value(b) % P
        got = call(h, "hs_fp30_sqr", a)
        assert got == model_product(value(a) ** 2), a
        got = call(h, "hs_fp30_mul_add2", a, b2, c, d)
        assert got == model_product(value(a) * value(b2) + value(c) * value(d)), (a, b2, c, d)
        assert abs(value(got)) <= P
        # norm on limbs of up to 3 * 2^29: sums and differences of three normalised operands
        s3 = [x + y - z for x, y, z in zip(a, b, c)]
        got = call(h, "hs_fp30_norm", s3)
        assert got == out_limbs(value(s3)), s3
        assert call(h, "hs_fp30_add", a, c) == [x + y for x, y in zip(a, c)]
        assert call(h, "hs_fp30_sub", a, c) == [x - y for x, y in zip(a, c)]
    for s in (3 * HALF, -3 * HALF):
        lim = [s] * 12 + [17 << 21]
        assert call(h, "hs_fp30_norm", lim) == out_limbs(value(lim))


def test_unpack_and_repack(libs):
    _, h = libs
    rnd = random.Random(32)
    edge = [0, 1, P - 1, (1 << 381) - 1 if (1 << 381) - 1 < P else P - 2, sum(1 << (W * j + 29) for j in range(12))]
    edge += [sum(((1 << W) - 1) << (W * j) for j in range(12)), sum((HALF - 1) << (W * j) for j in range(12))]
    for k in range(2000):
        v = edge[k] if k < len(edge) else rnd.randrange(P)
        words = (C.c_uint32 * 12)(*[(v >> (32 * i)) & 0xffffffff for i in range(12)])
        r = I32x13()
        h.hs_fp30_unpack(r, words)
        assert value(r) == v and all(abs(x) <= HALF for x in r), v
        # a product's output (|value| <= p) -> 14 x 28-bit limbs of value + p, normalised
        a = rand_operand(rnd, 1) if k >= 4 else [out_limbs(P), out_limbs(-P), [0] * N, out_limbs(P - 1)][k]
        o = (C.c_uint32 * 14)()
        h.hs_fp30_to_f28(o, I32x13(*a))
        assert sum(int(x) << (28 * j) for j, x in enumerate(o)) == value(a) + P
        assert all(x < 1 << 28 for x in o)


def _omul(o, p, k):
    r = C.create_string_buffer(144)
    kk = (C.c_uint64 * 4)(*[(k >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])
    o.og1_mul_raw(r, p, kk, 255)
    return r


def _aff(o, p):
    a = C.create_string_buffer(96)
    o.og1_to_affine(a, p)
    return a.raw


@pytest.fixture(scope="module")
def base_points(libs):
    o, h = libs
    rnd = random.Random(33)
    g = C.create_string_buffer(144)
    h.hs_g1_generator(g)
    return [_omul(o, g, rnd.randrange(1, R)) for _ in range(300)]


def _chain(h, pts, signs, at_inf, phi_at, form):
    r = C.create_string_buffer(144)
    h.hs_g1_madd_alt_chain_form.restype = C.c_int
    met = h.hs_g1_madd_alt_chain_form(r, b"".join(pts), bytes(signs), bytes(at_inf), len(pts), phi_at, form)
    return r, met


def test_chain_of_300_matches_the_28_bit_law(libs, base_points):
    o, h = libs
    rnd = random.Random(34)
    pts = [_aff(o, p) for p in base_points]
    signs = [rnd.randrange(2) for _ in pts]
    at_inf = [0] * len(pts)
    for i in (0, 7, 150, 151, 299):
        at_inf[i] = 1                      # entries at infinity: first, in the middle, around phi, last
    for phi_at in (151, 1, 300, 1000):     # in the middle; before the first addition; after the last; never crossed
        ref, _ = _chain(h, pts, signs, at_inf, phi_at, 0)
        assert not o.og1_is_inf(ref)
        for form in (1, 2):
            got, met = _chain(h, pts, signs, at_inf, phi_at, form)
            assert met == 0
            assert _aff(o, got) == _aff(o, ref), (phi_at, form)
    # without phi (phi on an empty accumulator is skipped) the chain is the plain signed sum
    head = 40
    ref = C.create_string_buffer(144)
    for p, s, z in zip(base_points[:head], signs, at_inf):
        if z:
            continue
        q = C.create_string_buffer(144)
        q.raw = p.raw
        if s:
            o.og1_neg(q, q)
        o.og1_add(ref, ref, q)
    # phi_at = 0: applied while the accumulator is still empty
    got, met = _chain(h, pts[:head], signs[:head], at_inf[:head], 0, 1)
    assert met == 0 and o.og1_equal(got, ref)
    # everything skipped: infinity
    got, met = _chain(h, pts[:5], signs[:5], [1] * 5, 2, 1)
    assert met == 0 and o.og1_is_inf(got)


def test_equal_x_leaves_zz_zero_and_the_fallback_is_exact(libs, base_points):
    o, h = libs
    rnd = random.Random(35)
    head, tail = 11, 9
    pts = [_aff(o, p) for p in base_points[:head + tail]]
    signs = [rnd.randrange(2) for _ in pts]
    run = C.create_string_buffer(144)      # the running sum after `head` entries
    for p, s in zip(base_points[:head], signs):
        q = C.create_string_buffer(144)
        q.raw = p.raw
        if s:
            o.og1_neg(q, q)
        o.og1_add(run, run, q)
    for same in (True, False):             # acc + (same point): doubling;  acc + (-point): infinity
        for rest in (tail, 0):             # in the middle of a chain, and as its last step
            mid_sign = 0 if same else 1
            cp = pts[:head] + [_aff(o, run)] + pts[head:head + rest]
            cs = signs[:head] + [mid_sign] + signs[head:head + rest]
            zi = [0] * len(cp)
            n = len(cp)
            ref, _ = _chain(h, cp, cs, zi, n, 0)
            _, met = _chain(h, cp, cs, zi, n, 1)
            assert met == 1, (same, rest)
            got, met = _chain(h, cp, cs, zi, n, 2)
            assert met == 1
            if rest == 0 and not same:
                assert o.og1_is_inf(got) and o.og1_is_inf(ref)
            else:
                assert not o.og1_is_inf(ref)
                assert _aff(o, got) == _aff(o, ref), (same, rest)
            # and the plain group law agrees (phi at the end of the chain: compare before it by undoing nothing --
            # phi_at = n applies phi to the whole sum, so check the phi-free chain too)
            exp = C.create_string_buffer(144)
            exp.raw = run.raw
            if same:
                o.og1_dbl(exp, exp)
            else:
                o.og1_neg(exp, exp)
                o.og1_add(exp, exp, run)
            for p, s in zip(base_points[head:head + rest], signs[head:head + rest]):
                q = C.create_string_buffer(144)
                q.raw = p.raw
                if s:
                    o.og1_neg(q, q)
                o.og1_add(exp, exp, q)
            got0, met = _chain(h, cp, cs, zi, 0, 2)
            assert met == 1 and o.og1_equal(got0, exp), (same, rest)


# ---- the op list of f30_test_ops.hpp on the shared corpora (tests/fp30_expect.py), as g++ builds it ----

def _host_ops(h):
    h.hs_f30_ops.restype = C.c_char_p
    return fx.parse_ops(h.hs_f30_ops().decode())


def test_op_list_is_the_one_the_law_relies_on(libs):
    _, h = libs
    assert _host_ops(h) == fx.REQUIRED_OPS


@pytest.mark.parametrize("k", range(len(fx.REQUIRED_OPS)), ids=lambda k: "%s%s" % fx.REQUIRED_OPS[k])
def test_op_on_its_corpus(libs, k):
    """every operation limb for limb against the model -- norm at LA = 1 and 2 (the other carry formula) included"""
    _, h = libs
    op = _host_ops(h)[k]
    cases = fx.field_cases(op)
    a, b, c, d = fx.pack_field(cases)
    out = (C.c_int32 * (14 * len(cases)))()
    assert h.hs_f30_run(k, out, a, b, c, d, len(cases)) == 0
    fx.check_field(op, cases, out)
    assert h.hs_f30_run(len(fx.REQUIRED_OPS), out, a, b, c, d, 1) == 1     # past the list


def _jac(pt):
    """affine integers -> the 144-byte Jacobian form of the oracle (2^384 domain, Z = 1)"""
    if pt is None:
        return bytes(144)
    r384 = pow(2, 384, P)
    return b"".join((v * r384 % P).to_bytes(48, "little") for v in (pt[0], pt[1], 1))


@pytest.fixture(scope="module")
def grp(libs):
    from test_gpu_dev_arith import Group
    return Group(*libs)


def test_step_model_is_the_group_law(grp):
    """the model of xyzz30_madd_alt, anchored without the code under test: the point an accumulator stands for (weights
    (1, 2, 0, 1), sign flag) moves by +-entry under the ORACLE's group law; equal x leaves ZZ = 0 mod p"""
    seen = set()
    for cl, st, inf, yneg, words, dneg, pt, (st2, inf2, yneg2) in fx.step_cases():
        seen.add(cl)
        before = None if inf else fx.state_point(st, bool(yneg))
        assert inf or before is not None
        entry = _jac(pt)
        want = grp.add(_jac(before), grp.neg(entry) if dneg else entry)
        assert not inf2
        after = fx.state_point(st2, yneg2)
        if cl == "equal_x":
            assert after is None and value(st2[2]) % P == 0
            assert pt[0] == before[0]
        else:
            assert after is not None and grp.equal(_jac(after), want), cl
            fx.check_state(st2)
    assert {"chain1", "chain2", "chain50", "shifted50", "empty", "equal_x"} <= seen


def test_phi_and_exit_models_are_the_group_law(grp):
    from arith_cases import LAMBDA
    mets = 0
    for st, phi, (words, met) in fx.state_cases():
        pt = fx.state_point(st, False)
        assert (pt is None) == bool(met)
        mets += met
        if pt is None:
            continue
        assert grp.equal(_jac(fx.state_point(phi, False)), grp.mul(_jac(pt), LAMBDA))
        x, y, zz, zzz = (sum(v << (28 * j) for j, v in enumerate(words[14 * i:14 * i + 14])) for i in range(4))
        assert (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P) == pt          # a point of one domain: 2^392 cancels
        assert pow(zz, 3, P) == zzz * zzz * pow(2, 392, P) % P                   # ZZ^3 = ZZZ^2, at 2^392
    assert mets


def test_step_phi_exit_match_the_model(libs):
    _, h = libs
    steps = fx.step_cases()
    n = len(steps)
    state = (C.c_int32 * (fx.STATE_WORDS * n))(*[v for s in steps for v in fx.flat_state(s[1])])
    flags = bytes(v for s in steps for v in (s[2], s[3], s[5]))
    entry = (C.c_uint32 * (fx.ENTRY_WORDS * n))(*[w for s in steps for w in s[4]])
    out, oflags = (C.c_int32 * (fx.STATE_WORDS * n))(), C.create_string_buffer(2 * n)
    h.hs_madd30_step(out, oflags, state, flags, entry, n)
    fx.check_steps(steps, list(out), oflags.raw)
    states = fx.state_cases()
    n = len(states)
    state = (C.c_int32 * (fx.STATE_WORDS * n))(*[v for s in states for v in fx.flat_state(s[0])])
    out = (C.c_int32 * (fx.STATE_WORDS * n))()
    h.hs_phi30(out, state, n)
    ex, met = (C.c_uint32 * (fx.EXIT_WORDS * n))(), C.create_string_buffer(n)
    h.hs_exit30(ex, met, state, n)
    fx.check_states(states, list(out), list(ex), met.raw)


def test_divergent_chains_are_the_group_law(libs, grp, base_points):
    """the 64 chains of the device's divergent launch, on the host: the 28-bit law and the 30-bit one with its fallback
    give the oracle's sum, phi included; the verdict is raised on the equal-x chain alone"""
    o, _ = libs
    pts = [grp.affine(p.raw) for p in base_points]
    chains = fx.divergent_chains(grp, pts)
    assert sorted(len(c[0]) for c in chains)[:3] == [0, 1, 2]
    mets = []
    for cp, cs, zi, phi_at in chains:
        want = fx.chain_expected(grp, cp, cs, zi, phi_at)
        for form in (0, 2):
            got, met = _chain(libs[1], [p[:96] for p in cp], cs, zi, phi_at, form)
            assert grp.equal(got.raw, want), (len(cp), phi_at, form)
        mets.append(met)
    assert mets == [1 if i == 9 else 0 for i in range(64)]


def test_generated_includes_are_the_generators_output():
    import sys
    csrc = os.path.join(ROOT, "c-kzg-4844_amd", "csrc")
    for mode, name in (("consts", "fp30_consts.inc"), ("cols", "fp30_asm_cols.inc")):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fp30_asm.py"), mode],
                             capture_output=True, text=True, check=True).stdout
        with open(os.path.join(csrc, name)) as f:
            assert f.read() == out, "%s is stale: python tools/gen_fp30_asm.py %s > c-kzg-4844_amd/csrc/%s" % (name, mode, name)
