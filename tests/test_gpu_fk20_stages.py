"""The two length-128 G1 transforms at the end of the FK20 proofs (fk20.hip: fk20_fft_stage_enqueue) read off the device
and compared with integers, in each of their six forms.

compute_cells_and_kzg_proofs and recover_cells_and_kzg_proofs reach the stage with the MSM sums of honest blobs: generic
points, which never meet an equal or an opposite operand, or -- the zero blob, a constant polynomial -- nothing but the
identity.  Here every input point is a_f * G with the scalars of tests/fk20_expect.py's corpus, in XYZZ form with a
random z that is not one, so every one of the 128 outputs of a transform is a known multiple of the generator:
out[k] = sum_{j < 64} w^(jk) sum_{f < 128} w^(-fj) a_f.  tests/test_fk20_expect_cpu.py shows that on this corpus every
addition site of every dataflow -- down to the step and the term of a multi-term sum -- meets a doubling, a
cancellation and an identity operand.

tests/native/fk20_shim.hip (libfk20_shim.so: its entry file linked with the product's own object files) runs the stage
on n transforms and says which form it took; n stands on both sides of every hand-over.  The corpus rotates through the
transforms, call after call until every vector has been there at that n, so the vectors on the two sides of every
multiple of 16 and 64 (the quad and wave padding edges) and at transform 0 and n - 1 (which the padding quads repeat)
differ.  EVERY output point is compared: X = x ZZ, Y = y ZZZ, ZZZ^2 = ZZ^3, the identity as the all-zero string and
nothing else.  The guard vector behind u comes back untouched, and the shim checks the guard behind the scratch.

The order of `out` is the natural order k: the expected points of the vectors that are not symmetric in k (the tones,
the deltas) are the oracle's multiples of the generator, and they are met at k, not at brp7(k).  The last test ties the
stage to the call: for the blob c x^64 + r(x), deg r < 64, every proof is compress([c] G), from the product on its FK20
path and from the oracle.  (Its FK20 input is NOT c G in every slot: u[f] = (c / 128) w^(66 f) X_63[f] with the whole
setup column X_63, generic points whose inverse transform is [c] G at j = 0, the identity at j = 1..63 and generic
above.  The corpus vector `fold_cancel` has that shape with known scalars; `const` is the all-equal input.)

Wall time per n on an MI355X, filling and comparison included (the module: 15 tests in 6.8 s, of which ~2.5 s make the
~7000 expected points once and ~1.5 s load the product and the oracle for the last test):
    n = 1: 0.48 s (30 calls)   8: 0.05 s   9: 0.05 s   16: 0.04 s   17: 0.04 s   48: 0.04 s   49: 0.05 s
    128: 0.11 s   129: 0.11 s   513: 0.39 s

profiles/fk20_stage_mutants.txt: four value-only mutants of the stage fail every case here and none of
tests/test_gpu_cells.py."""
import ctypes as C
import os
import random
import subprocess
import time

import pytest

import fk20_edge as fe
import fk20_expect as fx
import g1_expect as gx
from conftest import ROOT, ORACLE_SO

pytestmark = pytest.mark.gpu
R = gx.R
FK20_SHIM_SO = os.path.join(ROOT, "c-kzg-4844_amd", "libfk20_shim.so")
SIZES = [1, 8, 9, 16, 17, 48, 49, 128, 129, 513]
GUARD = bytes([0x5a]) * (128 * 192)


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(FK20_SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libfk20_shim.so"])
    lib = C.CDLL(FK20_SHIM_SO)
    lib.fks_transforms.restype = C.c_int
    return lib


_SRC = None


def source():
    """one G1Source for the module: k -> k G is memoised per scalar"""
    global _SRC
    if _SRC is None:
        if not os.path.exists(ORACLE_SO):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
        _SRC = gx.G1Source(C.CDLL(ORACLE_SO))
    return _SRC


@pytest.fixture(scope="module")
def material():
    """per corpus vector: its name, its 128 input points, the affine strings of its 128 expected outputs.  Computed
    once, shared by every n, never changed."""
    src = source()
    out = []
    for name, a in fx.corpus():
        want = fx.expect(a)
        out.append((name, [src.point(x) if x % R else gx.INF for x in a], [src.raw(e) for e in want]))
    return out


def layout(n, nvec):
    """calls x n vector indices: the corpus rotates through the transforms until every vector has appeared"""
    calls = (nvec + n - 1) // n
    return [[(c * n + i) % nvec for i in range(n)] for c in range(calls)]


def test_layout_covers_the_corpus_and_differs_at_the_edges():
    nvec = len(fx.corpus())
    assert nvec >= 26
    for n in SIZES:
        plan = layout(n, nvec)
        assert {v for row in plan for v in row} == set(range(nvec)), n
        for row in plan:
            if n > 1:
                assert row[0] != row[n - 1] and row[n - 1] != row[n - 2], n
            for edge in range(16, n, 16):   # (every multiple of 64 is one of 16)
                assert row[edge - 1] != row[edge], (n, edge)


@pytest.mark.parametrize("n", SIZES)
def test_every_output_of_every_form_on_chosen_points(shim, material, n):
    t0 = time.time()
    rnd = random.Random(n)
    nvec = len(material)
    bad = []
    for call, row in enumerate(layout(n, nvec)):
        buf = bytearray((n + 1) * 128 * 192)
        for i, v in enumerate(row):
            pts = material[v][1]
            o = i * 128 * 192
            buf[o:o + 128 * 192] = b"".join(gx.xyzz_raw(pt, rnd.randrange(2, gx.P)) for pt in pts)
        buf[n * 128 * 192:] = GUARD
        data = (C.c_uint8 * len(buf)).from_buffer(buf)
        form, rc = C.c_int(-1), C.c_int(-1)
        ret = shim.fks_transforms(data, C.c_size_t(n), C.byref(form), C.byref(rc))
        assert ret == 0 and rc.value == 0, (n, call, ret, rc.value)
        assert form.value == fx.form_of(n), (n, fx.FORM_NAMES[form.value])
        assert bytes(buf[n * 128 * 192:]) == GUARD, "the stage wrote behind its n transforms"
        got = bytes(buf)
        for i, v in enumerate(row):
            name, _, want = material[v]
            wrong = [k for k in range(128) if not gx.xyzz_is(got[(i * 128 + k) * 192:(i * 128 + k + 1) * 192], want[k])]
            if wrong:
                bad.append((call, i, name, wrong[:8], len(wrong)))
    print("n = %d (%s): %d calls, %.2f s" % (n, fx.FORM_NAMES[fx.form_of(n)], len(layout(n, nvec)), time.time() - t0))
    assert not bad, "n = %d, form %s: (call, transform, vector, first wrong k, how many) %r" % (
        n, fx.FORM_NAMES[fx.form_of(n)], bad[:12])


def test_the_output_order_is_the_natural_one(material):
    """what the comparison above rests on: the expected outputs of tone_1 differ at k and brp7(k), so a stage that
    left its output bit-reversed would not pass"""
    by = {name: want for name, _, want in material}
    want = by["tone_1"]
    assert sum(1 for k in range(128) if want[k] != want[fx.brp7(k)]) >= 100
    assert want[1] == source().raw(128 * fx.A * fx.W[1] % R)


def test_the_shim_refuses_what_it_does_not_serve(shim):
    form, rc = C.c_int(-1), C.c_int(-1)
    buf = (C.c_uint8 * 192)()
    for n in (0, 641, 1 << 20):
        assert shim.fks_transforms(buf, C.c_size_t(n), C.byref(form), C.byref(rc)) == 9998
    assert rc.value == -1 and form.value == -1


def blob_of(poly):
    ev = fe._ntt(poly, fe.W4096)
    return b"".join(ev[fe._brp(i, 12)].to_bytes(32, "big") for i in range(4096))


@pytest.mark.parametrize("c", [0x1234567 * 0x89abcdef % R, R - 1])
def test_a_blob_whose_proofs_are_all_c_times_g(hip_fk20, oracle, c):
    """p(x) = c x^64 + r(x) with deg r < 64: the quotient by x^64 - h^64 is the constant c for every coset, so all 128
    proofs are compress([c] G), whatever r is.  The product on its FK20 path (direct_max = 0) and the oracle both say
    so.  On the way 63 of the 64 fold additions cancel and the forward pass runs on one point among identities."""
    rnd = random.Random(c)
    poly = [rnd.randrange(R) for _ in range(64)] + [c] + [0] * (4096 - 65)
    blob = blob_of(poly)
    want = source().compressed(c)
    cells, proofs = hip_fk20.compute_cells_and_kzg_proofs(blob)
    ecells, eproofs = oracle.compute_cells_and_kzg_proofs(blob)
    assert list(proofs) == [want] * 128
    assert list(eproofs) == [want] * 128
    assert list(cells) == list(ecells)
