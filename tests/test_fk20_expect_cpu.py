"""What can be said about the FK20 transform stage without a GPU (tests/fk20_expect.py, fk20_fft_plan.hpp).

The reference of tests/test_gpu_fk20_stages.py by a second route; the replay of each of the three dataflows of the
device against it on every vector of the corpus; and the COVERAGE CONDITION that makes the GPU test mean something: over
the corpus, every addition site of every dataflow meets an equal operand (a doubling), an opposite operand (a
cancellation) and an identity operand at least once.  It holds twice: for the site classes as such (radix-2 addsub per
stage and the fold, each radix-4 site, each V, each post sum and the fold of radix-8) and for every site down to the
step and the term of a multi-term sum.  No (site, class) pair is excepted: the pairs the vectors built from one scalar
cannot reach are reached by the solved vectors (fk20_expect.solve_sites).

The plan header through libhost_shim.so: six forms with the hand-overs at 8|9, 16|17, 48|49, 128|129, 512|513, and a
scratch size that grows with n inside a form."""
import ctypes as C
import os
import subprocess

import pytest

import fk20_expect as fx
from conftest import ROOT, SHIM_SO

PKG = os.path.join(ROOT, "c-kzg-4844_amd")
R = fx.R
KINDS = ("r2", "r4", "r8")
# (site class, class) pairs that structurally cannot occur, by name with the reason: none.  The list may never exceed a
# quarter of the pairs of a dataflow: beyond that the corpus is extended instead.
STRUCTURALLY_IMPOSSIBLE = {"r2": {}, "r4": {}, "r8": {}}


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    lib.hs_fk20_fft_form.restype = C.c_int
    lib.hs_fk20_fft_scratch_bytes.restype = C.c_uint64
    return lib


@pytest.fixture(scope="module")
def vectors():
    return fx.corpus()


def test_the_corpus_holds_the_named_vectors(vectors):
    names = [n for n, _ in vectors]
    assert len(set(names)) == len(names)
    want = ["random", "const", "halves", "zero", "fold_cancel"] + ["delta_%d" % f for f in (0, 1, 64, 127)]
    want += ["tone_%d" % m for m in (0, 1, 2, 16, 32, 63, 64, 65, 96, 127)] + ["small_%d" % s for s in range(8)]
    assert set(want) <= set(names)
    assert fx.A % R != 0
    by = dict(vectors)
    assert all(len(a) == 128 and all(0 <= x < R for x in a) for a in by.values())
    assert by["const"] == [fx.A] * 128 and by["zero"] == [0] * 128
    assert by["delta_64"][64] == fx.A and sum(1 for x in by["delta_64"] if x) == 1
    assert all(set(by["small_%d" % s]) <= {0, fx.A, R - fx.A, 2 * fx.A % R, -2 * fx.A % R} for s in range(8))


def test_reference_by_a_second_route(vectors):
    for name, a in vectors:
        assert fx.expect(a) == fx.expect_naive(a), name


def test_what_the_reference_says_about_the_structured_vectors(vectors):
    by = dict(vectors)
    a = fx.A
    assert fx.expect(by["zero"]) == [0] * 128
    assert fx.expect(by["const"]) == [128 * a % R] * 128          # 128 a at j = 0, spread over every k
    for m in fx.TONES:
        out = fx.expect(by["tone_%d" % m])
        if m >= 64:   # the truncation removes it: the identity everywhere, reached from points that are not
            assert out == [0] * 128, m
        else:
            assert out == [128 * a * fx.W[(m * k) % 128] % R for k in range(128)], m
    assert fx.expect(by["fold_cancel"]) == [128 * a % R] * 128 and len(set(by["fold_cancel"])) == 128
    ev = fx.Events()
    for kind in KINDS:   # 63 of the 64 fold additions cancel, in every dataflow
        fx.REPLAYS[kind](by["fold_cancel"], ev)
        assert ev.count[((kind, "fold"), "opposite")] == 63
    for m in fx.TONES:   # m even: u[f + 64] = u[f]; m odd: u[f + 64] = -u[f]
        t = by["tone_%d" % m]
        assert all((t[f + 64] - (t[f] if m % 2 == 0 else -t[f])) % R == 0 for f in range(64))


@pytest.mark.parametrize("kind", KINDS)
def test_replay_reproduces_the_reference(vectors, kind):
    for name, a in vectors:
        trace = []
        out, _ = fx.REPLAYS[kind](a, trace=trace)
        assert out == fx.expect(a), (kind, name)
        assert trace[-1][1] == out


@pytest.mark.parametrize("kind", KINDS)
def test_every_site_class_meets_every_operand_class(vectors, kind):
    """the coverage condition"""
    classes = fx.sites(kind, fx.CLASS_DEPTH[kind])
    assert len(classes) == {"r2": 25, "r4": 19, "r8": 8}[kind]
    excepted = STRUCTURALLY_IMPOSSIBLE[kind]
    assert 4 * len(excepted) <= 3 * len(classes)     # a quarter of the (site, class) pairs
    _, cov = fx.coverage(kind, vectors)
    for site in classes:
        for cls in fx.CLASSES:
            if (site, cls) in excepted:
                assert cov[(site, cls)] == 0, "listed as impossible, yet met: %r" % ((site, cls),)
            else:
                assert cov[(site, cls)] >= 1, (site, cls)


@pytest.mark.parametrize("kind", KINDS)
def test_every_step_and_term_meets_every_operand_class(vectors, kind):
    """the same for every site down to its step and its term: 25, 55 and 59 of them"""
    assert len(fx.sites(kind, fx.FINE_DEPTH)) == {"r2": 25, "r4": 55, "r8": 59}[kind]
    assert fx.missing(kind, vectors, fx.FINE_DEPTH) == []


def test_the_events_are_classified_as_they_are_named():
    ev = fx.Events()
    cases = [(3, 3, False, "equal"), (3, R - 3, False, "opposite"), (3, 3, True, "opposite"), (3, R - 3, True, "equal"),
             (0, 5, False, "left"), (5, 0, True, "right"), (0, 0, False, "both"), (1, 2, False, "plain")]
    for x, y, neg, kind in cases:
        before = ev.count[(("s",), kind)]
        assert ev.add(("s",), x, y, neg) == (x - y if neg else x + y) % R
        assert ev.count[(("s",), kind)] == before + 1
    assert ev.by_class(1) == {(("s",), "equal"): 2, (("s",), "opposite"): 2, (("s",), "identity"): 3}


def test_six_forms_with_the_handovers_of_the_plan_header(shim):
    form = lambda n: shim.hs_fk20_fft_form(C.c_uint64(n))
    assert [form(n) for n in (1, 8, 9, 16, 17, 48, 49, 128, 129, 512, 513, 4096)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    changes = [n for n in range(1, 1025) if form(n) != form(n + 1)]
    assert changes == [8, 16, 48, 128, 512] == list(fx.HANDOVERS)
    assert all(form(n) == fx.form_of(n) for n in range(1, 1025))
    assert len(fx.FORM_NAMES) == len(fx.FORM_REPLAY) == 6


def test_scratch_bytes_grow_with_n_inside_a_form(shim):
    sb = lambda n: shim.hs_fk20_fft_scratch_bytes(C.c_uint64(n))
    for n in range(1, 640):
        if fx.form_of(n) == fx.form_of(n + 1):
            assert sb(n) <= sb(n + 1), n
            if fx.form_of(n) <= 3:
                assert sb(n) < sb(n + 1), n
    assert all(sb(n) == 0 for n in (129, 512, 513, 640))            # radix-2 works in place
    assert all(sb(n) % 256 == 0 for n in range(1, 200))
    # radix-8: two buffers of n x 128 raw records of 57 words and n x 336 ladder results; radix-4: n x (128 + 160) points
    al = lambda v: (v + 255) // 256 * 256
    assert sb(5) == 2 * al(5 * 128 * 228) + al(5 * 336 * 228)
    assert sb(100) == al(100 * 128 * 192) + al(100 * 160 * 192)


def test_make_all_builds_the_fk20_shim():
    with open(os.path.join(PKG, "Makefile")) as f:
        text = f.read()
    all_line = next(line for line in text.splitlines() if line.startswith("all:"))
    assert "libfk20_shim.so" in all_line.split()
    rule = next(line for line in text.splitlines() if line.startswith("libfk20_shim.so:"))
    assert "$(OBJS)" in rule
    so = os.path.join(PKG, "libfk20_shim.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", PKG, "-j", "8", "libfk20_shim.so"])
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "fks_transforms" in names
    assert any("fk20_fft_stage_enqueue" in s for s in names)   # the product's stage function, from the product's objects
