"""tests/coset_expect.py by second routes: blob sizes 16 and 64 (extended 32 and 128), every coset size l up to half the
blob size, a known secret.  The definition against the division identity and the interpolant; the strided FK20 layout
against the definition; the ladder between sizes; the bit-reversed sub-coset structure; the first half of l = 1 against
the domain call's model."""
import random

import pytest

import coset_expect as E
import domain_expect as D

R = D.R
SIZES = [(N, l) for N in (16, 64) for l in (1 << e for e in range(0, E.log2(N))) if l <= N // 2]


def _polys(N, rnd):
    return [[rnd.randrange(R) for _ in range(N)],
            [0] * N, [5] + [0] * (N - 1),
            [0] * (N - 1) + [1],
            [rnd.randrange(R) for _ in range(N - 1)] + [R - 1]]


def test_the_sizes_are_the_ones_the_issue_names():
    assert [l for N, l in SIZES if N == 16] == [1, 2, 4, 8]
    assert [l for N, l in SIZES if N == 64] == [1, 2, 4, 8, 16, 32]


@pytest.mark.parametrize("N,l", SIZES)
def test_definition_by_the_division_identity(N, l):
    """p(s) = q_c(s) (s^l - a) + r_c(s), deg r_c < l, and r_c = p on the coset"""
    rnd = random.Random(N * 100 + l)
    s = rnd.randrange(2, R)
    for p in _polys(N, rnd):
        pi = E.openings_by_definition(p, s, N, l)
        assert len(pi) == 2 * N // l
        for c in range(2 * N // l):
            pts = E.coset_points(N, l, c)
            a = pow(pts[0], l, R)
            assert all(pow(x, l, R) == a for x in pts) and len(set(pts)) == l
            r = E.remainder(p, l, a)
            assert len(r) <= l
            assert (pi[c] * (pow(s, l, R) - a) + E.evaluate(r, s)) % R == E.evaluate(p, s)
            for x in pts:
                assert E.evaluate(r, x) == E.evaluate(p, x)


@pytest.mark.parametrize("N,l", SIZES)
def test_layout_against_the_definition(N, l):
    rnd = random.Random(N * 100 + l + 7)
    s = rnd.randrange(2, R)
    k = N // l
    polys = _polys(N, rnd) + [[1, 2, 3][:l] + [0] * (N - min(l, 3)),   # degree < l: every opening is the identity
                              [0] * l + [1] + [0] * (N - l - 1)]       # X^l: every opening is [1]
    for p in polys:
        assert E.h_by_layout(p, s, N, l) == E.h_by_definition(p, s, N, l)
        assert E.openings_by_layout(p, s, N, l) == E.openings_by_definition(p, s, N, l)
    assert E.openings_by_layout(polys[1], s, N, l) == [0] * (2 * k) == E.openings_by_layout(polys[2], s, N, l)
    assert E.openings_by_layout(polys[-2], s, N, l) == [0] * (2 * k)
    assert E.openings_by_layout(polys[-1], s, N, l) == [1] * (2 * k)


@pytest.mark.parametrize("N,l", SIZES)
def test_index_maps_against_the_columns(N, l):
    e = E.log2(l)
    k = N // l
    p = list(range(1, N + 1))
    flat = [x for col in E.circulant_columns(p, l) for x in col]
    assert len(flat) == 2 * N
    for t in range(2 * N):
        src = E.circulant_source(t, e, N)
        assert (p[src] if src >= 0 else 0) == flat[t]
    s = 3
    xs = [x for col in E.setup_columns(s, N, l) for x in col]
    used = set()
    for t in range(2 * N):
        src = E.setup_source(t, e, N)
        assert (pow(s, src, R) if src >= 0 else 0) == xs[t]
        if src >= 0:
            assert 0 <= src < N - l and src not in used
            used.add(src)
    assert len(used) == l * (k - 1)
    # every coefficient from l upward is read exactly once, none below
    reads = sorted(E.circulant_source(t, e, N) for t in range(2 * N) if E.circulant_source(t, e, N) >= 0)
    assert reads == list(range(l, N))


def test_size_one_is_the_single_point_form():
    for N in (16, 64):
        rnd = random.Random(N)
        s, p = rnd.randrange(2, R), [rnd.randrange(R) for _ in range(N)]
        assert E.circulant_columns(p, 1) == [D.circulant(p)]
        assert E.setup_columns(s, N, 1) == [D.setup_vector(s, N)]
        # the first half of the extended domain in bit-reversed order is the blob's own domain in its order
        assert E.brp_roots(2 * N)[:N] == E.brp_roots(N)
        by_domain = D.openings_by_definition(p, s, N)   # natural order of the N-th roots
        got = E.openings_by_layout(p, s, N, 1)
        assert got[:N] == [by_domain[D.brp(j, E.log2(N))] for j in range(N)]
        # the outer half: quotient at a point outside the blob's domain, pi (s - x) = p(s) - p(x)
        for j in range(N, 2 * N):
            x = E.brp_roots(2 * N)[j]
            assert got[j] * (s - x) % R == (E.evaluate(p, s) - E.evaluate(p, x)) % R


@pytest.mark.parametrize("N", [16, 64])
def test_ladder_between_the_sizes(N):
    rnd = random.Random(N + 1)
    s, p = rnd.randrange(2, R), [rnd.randrange(R) for _ in range(N)]
    level = E.openings_by_definition(p, s, N, 1)
    l = 2
    while l <= N // 2:
        level = E.ladder_step(level, N, l)
        assert level == E.openings_by_definition(p, s, N, l) == E.openings_by_layout(p, s, N, l), l
        l *= 2


@pytest.mark.parametrize("N,l", [x for x in SIZES if x[1] > 1])
def test_sub_coset_structure(N, l):
    """coset c of size l is cosets 2c and 2c + 1 of size l / 2, whose l/2-th powers are a and -a"""
    for c in range(2 * N // l):
        lo, hi = E.coset_points(N, l // 2, 2 * c), E.coset_points(N, l // 2, 2 * c + 1)
        assert E.coset_points(N, l, c) == lo + hi
        a = pow(lo[0], l // 2, R)
        assert all(pow(x, l // 2, R) == a for x in lo) and all(pow(x, l // 2, R) == R - a for x in hi)
        assert a * a % R == pow(E.coset_points(N, l, c)[0], l, R)


def test_extended_evaluations_of_a_blob():
    rnd = random.Random(3)
    c = [rnd.randrange(R) for _ in range(5)]
    ev, z = E.ext_evaluations(c), E.ext_domain_points()
    for j in (0, 1, 4095, 4096, 8191):
        assert ev[j] == E.evaluate(c, z[j])
    assert b"".join(v.to_bytes(32, "big") for v in ev[:4096]) == D.blob_of_poly(c)
