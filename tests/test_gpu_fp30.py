"""Fp on 13 signed 30-bit limbs (fp30.hpp) and the accumulate loop's mixed addition on it (g1_30.hpp) as the DEVICE runs
them -- the plain bodies as the device compiler builds them and the generated inline-asm products (fp30_asm_cols.inc,
under CKZG_F28_ASM_BLOCKS: what k_msm_accumulate<256, false> runs) -- through tests/native/dev_shim.hip (ds_plain_* /
ds_asm_*), limb for limb against the Python-integer models of tests/fp30_expect.py on its corpora: operands, limbs,
quotient digits and result digits at the ends of their ranges, the fullest columns, accumulators at their declared
bounds.  No tolerance and no reduction mod p before comparing; nothing is skipped or filtered.

Geometry as in tests/test_gpu_dev_arith.py: every list runs whole in workgroups of 256 and its first 101 items (every
class is among them) in workgroups of 64.  The chains run one thread each; the divergent launch puts 64 chains of
different lengths, phi positions and fates into one wave.  After any non-zero return of a shim call nothing more is
launched (DevShim)."""
import ctypes as C
import os
import random
import subprocess

import pytest

import fp30_expect as fx
from arith_cases import R
from conftest import ORACLE_SO, ROOT, SHIM_SO
from test_gpu_dev_arith import DEV_SHIM_SO, FORMS, DevShim, Group

pytestmark = pytest.mark.gpu

# every exported function this module binds, once per form (tests/test_dev_shim_cpu.py checks the library for them)
SHIM_FUNCTIONS_30 = ["f30_ops", "f30field", "madd30_step", "phi30", "exit30", "g1_chain30"]


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
        getattr(d, "ds_%s_f30_ops" % form).restype = C.c_char_p
    return Group(o, h), DevShim(d)


def _geometries(n):
    return ((n, 256), (min(n, fx.SUBSET_LEN), 64))


@pytest.mark.parametrize("form", FORMS)
def test_op_list(env, form):
    _, shim = env
    assert fx.parse_ops(getattr(shim.lib, "ds_%s_f30_ops" % form)().decode()) == fx.REQUIRED_OPS


@pytest.mark.parametrize("k", range(len(fx.REQUIRED_OPS)), ids=lambda k: "%s%s" % fx.REQUIRED_OPS[k])
@pytest.mark.parametrize("form", FORMS)
def test_field_op(env, form, k):
    _, shim = env
    op = fx.REQUIRED_OPS[k]
    cases = fx.field_cases(op)
    a, b, c, d = fx.pack_field(cases)
    for count, block in _geometries(len(cases)):
        out = (C.c_int32 * (14 * len(cases)))()
        shim.call(form, "f30field", k, out, a, b, c, d, count, block)
        fx.check_field(op, cases, out, count)
        assert not any(out[14 * count:])          # nothing is written past the items asked for


@pytest.mark.parametrize("form", FORMS)
def test_madd30_step(env, form):
    _, shim = env
    steps = fx.step_cases()
    n = len(steps)
    state = (C.c_int32 * (fx.STATE_WORDS * n))(*[v for s in steps for v in fx.flat_state(s[1])])
    flags = bytes(v for s in steps for v in (s[2], s[3], s[5]))
    entry = (C.c_uint32 * (fx.ENTRY_WORDS * n))(*[w for s in steps for w in s[4]])
    for count, block in _geometries(n):
        out, oflags = (C.c_int32 * (fx.STATE_WORDS * n))(), C.create_string_buffer(2 * n)
        shim.call(form, "madd30_step", out, oflags, state, flags, entry, count, block)
        fx.check_steps(steps, list(out), oflags.raw, count)


@pytest.mark.parametrize("form", FORMS)
def test_phi30_and_exit30(env, form):
    _, shim = env
    states = fx.state_cases()
    n = len(states)
    state = (C.c_int32 * (fx.STATE_WORDS * n))(*[v for s in states for v in fx.flat_state(s[0])])
    for count, block in _geometries(n):
        out = (C.c_int32 * (fx.STATE_WORDS * n))()
        shim.call(form, "phi30", out, state, count, block)
        ex, met = (C.c_uint32 * (fx.EXIT_WORDS * n))(), C.create_string_buffer(n)
        shim.call(form, "exit30", ex, met, state, count, block)
        fx.check_states(states, list(out), list(ex), met.raw, count)


# ---- chains ----

@pytest.fixture(scope="module")
def base_points(env):
    grp, _ = env
    rnd = random.Random(33)
    return [grp.affine(grp.mul(grp.g, rnd.randrange(1, R))) for _ in range(300)]


def _run_chains(shim, form, chains, kind, block):
    """chains: [(points, signs, at_inf, phi_at)] -> ([point], [met]) of one launch"""
    n = len(chains)
    start = [0]
    for c in chains:
        start.append(start[-1] + len(c[0]))
    pts = b"".join(p for c in chains for p in c[0])
    signs = bytes(s for c in chains for s in c[1])
    at_inf = bytes(z for c in chains for z in c[2])
    out, met = C.create_string_buffer(144 * n), C.create_string_buffer(n)
    shim.call(form, "g1_chain30", kind, out, met, pts, signs, at_inf, (C.c_uint32 * (n + 1))(*start),
              (C.c_uint32 * n)(*[c[3] for c in chains]), n, block)
    return [out.raw[144 * i:144 * i + 144] for i in range(n)], list(met.raw)


@pytest.mark.parametrize("form", FORMS)
def test_chain_of_300(env, base_points, form):
    """the chains of tests/test_fp30_cpu.py, one per phi position: the 30-bit law gives the 28-bit law's affine point
    and raises no verdict -- a spurious one would only cost the product time, and no other test would see it"""
    grp, shim = env
    pts, signs, at_inf, phis = fx.chain_300(grp, base_points)
    chains = [(pts, signs, at_inf, phi_at) for phi_at in phis]
    ref, met0 = _run_chains(shim, form, chains, 0, 64)
    assert met0 == [0] * len(chains)
    for c, r in zip(chains, ref):
        assert not grp.is_inf(r) and grp.equal(r, fx.chain_expected(grp, *c)), c[3]
    for kind in (1, 2):
        got, met = _run_chains(shim, form, chains, kind, 64)
        assert met == [0] * len(chains), kind
        for c, r, g in zip(chains, ref, got):
            assert grp.affine(g) == grp.affine(r), (kind, c[3])


@pytest.mark.parametrize("form", FORMS)
def test_equal_x_chains(env, base_points, form):
    """acc + its own point (doubling) and acc + its negative (infinity), mid-chain and as the last step: the exit says
    so, and with the fallback the sum is the oracle's"""
    grp, shim = env
    chains = []
    for cp, cs, zi in fx.equal_x_chains(grp, base_points):
        chains += [(cp, cs, zi, len(cp)), (cp, cs, zi, 0)]
    want = [fx.chain_expected(grp, *c) for c in chains]
    assert sum(grp.is_inf(w) for w in want) == 2             # the cancellation as the last step, with and without phi
    _, met = _run_chains(shim, form, chains, 1, 64)
    assert met == [1] * len(chains)
    got, met = _run_chains(shim, form, chains, 2, 64)
    assert met == [1] * len(chains)
    ref, _ = _run_chains(shim, form, chains, 0, 64)
    for i, w in enumerate(want):
        assert grp.equal(got[i], w) and grp.equal(ref[i], w), i
        assert grp.affine(got[i]) == grp.affine(ref[i]), i


@pytest.mark.parametrize("form", FORMS)
def test_divergent_launch(env, base_points, form):
    """64 chains in one wave: lengths 0, 1, 2 and up, one all at infinity, one with an equal-x step, a phi position each
    -- the lanes part at entry, at phi and at exit, as the product's do.  Every chain is right."""
    grp, shim = env
    chains = fx.divergent_chains(grp, base_points)
    assert len(chains) == 64
    want = [fx.chain_expected(grp, *c) for c in chains]
    verdicts = [1 if i == 9 else 0 for i in range(64)]
    for kind in (0, 1, 2):
        got, met = _run_chains(shim, form, chains, kind, 64)
        assert met == ([0] * 64 if kind == 0 else verdicts), kind
        for i, w in enumerate(want):
            if kind == 1 and verdicts[i]:
                continue                                     # without the fallback that lane holds no point
            assert grp.equal(got[i], w), (kind, i, len(chains[i][0]), chains[i][3])
