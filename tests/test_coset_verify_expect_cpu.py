"""tests/coset_verify_expect.py by second routes, on a blob of N = 64 coefficients (extended domain of 128 points) at
every coset size 2^e, e <= 6, with a known secret: the interpolation coefficients against evaluating I at the l points;
the identity of an item against the openings by definition (tests/coset_expect.py); the order of the points against
coset_expect.coset_points; the batch identity against the items' own, and its soundness against a pair of errors that
cancel under equal weights; the aggregate route to sum r^i I_i against the per-item one."""
import hashlib
import random

import pytest

import coset_expect as E
import coset_verify_expect as V
import domain_expect as D

R = D.R
N = 64
ES = list(range(7))


def _setup(e, seed):
    rnd = random.Random(1000 * e + seed)
    s = rnd.randrange(2, R)
    p = [rnd.randrange(R) for _ in range(N)]
    l = 1 << e
    pis = E.openings_by_definition(p, s, N, l)
    items = []
    for c in range(2 * N // l):
        ys = [E.evaluate(p, x) for x in E.coset_points(N, l, c)]
        items.append((E.evaluate(p, s), c, ys, pis[c]))
    return rnd, s, p, items


@pytest.mark.parametrize("e", ES)
def test_points_are_in_the_order_of_the_interface(e):
    l, w = 1 << e, D.root_of_unity(2 * N)
    wl = pow(w, 2 * N // l, R)
    for c in range(V.cosets(e, N)):
        x = V.x_of(c, e, N)
        assert [x * pow(wl, D.brp(j, e), R) % R for j in range(l)] == E.coset_points(N, l, c)
        assert pow(x, l, R) == pow(w, V.shift_root(c, e, N), R)
        for k in range(l):
            assert pow(x, -k, R) == pow(w, V.unshift_root(c, e, k, N), R)


@pytest.mark.parametrize("e", ES)
def test_coefficients_interpolate_the_values(e):
    rnd = random.Random(e)
    l = 1 << e
    for c in (0, 1, V.cosets(e, N) - 1):
        ys = [rnd.randrange(R) for _ in range(l)]
        a = V.interp_coeffs(ys, c, e, N)
        assert len(a) == l
        assert [E.evaluate(a, x) for x in E.coset_points(N, l, c)] == ys
        # stage 4 alone leaves the coset factor in: a_k = col_k x_c^-k
        col = V.column_coeffs(ys, e, N)
        assert [v * pow(V.x_of(c, e, N), -k, R) % R for k, v in enumerate(col)] == a
    assert V.interp_coeffs([0] * l, 0, e, N) == [0] * l
    assert V.interp_coeffs([7] * l, 1, e, N) == [7] + [0] * (l - 1)


@pytest.mark.parametrize("e", ES)
def test_column_transform_by_butterflies(e):
    """the route of the kernel: e stages, every position makes its own output with the twiddle of the index map"""
    rnd = random.Random(50 + e)
    l, w = 1 << e, D.root_of_unity(2 * N)
    ys = [rnd.randrange(R) for _ in range(l)]
    v = list(ys)
    for s in range(1, e + 1):
        half = 1 << (s - 1)
        tw = [pow(w, V.twiddle_root(k, s, N), R) for k in range(l)]
        v = [(v[k ^ half] - v[k] * tw[k]) % R if k & half else (v[k] + v[k ^ half] * tw[k]) % R for k in range(l)]
    assert [x * pow(l, -1, R) % R for x in v] == V.column_coeffs(ys, e, N)


@pytest.mark.parametrize("e", ES)
def test_identity_of_an_item_against_the_definition(e):
    rnd, s, p, items = _setup(e, 1)
    l = 1 << e
    for cm, c, ys, pi in items:
        assert V.item_holds(cm, c, ys, pi, s, e, N)
    cm, c, ys, pi = items[1]
    j = rnd.randrange(l)
    assert not V.item_holds(cm, c, ys[:j] + [(ys[j] + 1) % R] + ys[j + 1:], pi, s, e, N)
    assert not V.item_holds(cm, c, ys, (pi + 1) % R, s, e, N)
    assert not V.item_holds((cm + 1) % R, c, ys, pi, s, e, N)
    assert not V.item_holds(cm, 0, ys, pi, s, e, N)                      # the neighbouring coset
    if N - l > l:   # (a quotient of degree below l does not depend on the coset: every proof is the same)
        assert not V.item_holds(cm, c, ys, items[0][3], s, e, N)         # the neighbour's proof


@pytest.mark.parametrize("e", ES)
def test_batch_identity(e):
    rnd, s, p, items = _setup(e, 2)
    # a second polynomial, so that two commitments are interleaved
    p2 = [rnd.randrange(R) for _ in range(N)]
    l = 1 << e
    pis2 = E.openings_by_definition(p2, s, N, l)
    other = [(E.evaluate(p2, s), c, [E.evaluate(p2, x) for x in E.coset_points(N, l, c)], pis2[c]) for c in range(2 * N // l)]
    mixed = [it for pair in zip(items, other) for it in pair] + [items[0], items[0]]
    r = rnd.randrange(2, R)
    assert V.batch_holds(mixed, r, s, e, N)
    # the aggregate route to sum r^i I_i against the items' own polynomials
    rp = [pow(r, i, R) for i in range(len(mixed))]
    direct = [0] * l
    for pw, it in zip(rp, mixed):
        for k, a in enumerate(V.interp_coeffs(it[2], it[1], e, N)):
            direct[k] = (direct[k] + pw * a) % R
    assert V.interp_sum(V.aggregate(mixed, rp, e, N), e, N) == direct
    # one false item makes the batch false
    cm, c, ys, pi = mixed[3]
    forged = mixed[:3] + [(cm, c, [(ys[0] + 1) % R] + ys[1:], pi)] + mixed[4:]
    assert not V.batch_holds(forged, r, s, e, N)


@pytest.mark.parametrize("e", ES)
def test_errors_that_cancel_under_equal_weights_do_not_cancel_under_powers_of_r(e):
    rnd, s, p, items = _setup(e, 3)
    cm, c, ys, pi = items[1]
    j, delta = rnd.randrange(1 << e), rnd.randrange(1, R)
    up = (cm, c, ys[:j] + [(ys[j] + delta) % R] + ys[j + 1:], pi)
    down = (cm, c, ys[:j] + [(ys[j] - delta) % R] + ys[j + 1:], pi)
    assert V.batch_holds([up, down], 1, s, e, N)          # equal weights: the forgery goes through
    assert not V.batch_holds([up, down], rnd.randrange(2, R), s, e, N)


def test_transcript_layout():
    c0, c1 = b"\xc0" + bytes(47), b"\x80" + bytes(46) + b"\x01"
    for e in ES:
        ev = [bytes([i]) * (32 << e) for i in range(3)]
        t = V.transcript([c0, c1, c0], [5, 0, 5], ev, [c1, c1, c0], e)
        assert t[:16] == b"RCKZGCBATCH__V1_"
        assert [int.from_bytes(t[16 + 8 * i:24 + 8 * i], "big") for i in range(4)] == [4096, 1 << e, 2, 3]
        assert t[48:144] == c0 + c1
        per = 16 + (32 << e) + 48
        assert len(t) == 144 + 3 * per
        second = t[144 + per:144 + 2 * per]
        assert second == (1).to_bytes(8, "big") + (0).to_bytes(8, "big") + ev[1] + c1
        want = int.from_bytes(hashlib.sha256(t).digest(), "big") % R
        assert V.challenge([c0, c1, c0], [5, 0, 5], ev, [c1, c1, c0], e) == want
