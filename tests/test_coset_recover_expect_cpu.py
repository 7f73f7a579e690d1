"""The model of tests/coset_recover_expect.py checked against itself by other routes, so that the product is never
compared with a single derivation: the direct products against the coefficients of prod (y - root) evaluated by Horner
(e >= 4), against the closed forms of the two half sets at every e, and against the cell model's numbers at e = 6; the
slices, the picker and the plan on cases small enough to read."""
import random

import pytest

import coset_recover_expect as X
from coset_recover_expect import R

ES = list(range(7))


def _sample(e, extra=()):
    m = X.cosets(e)
    rnd = random.Random(100 + e)
    return sorted(set([0, 1, m // 2 - 1, m // 2, m - 1] + list(extra) + [rnd.randrange(m) for _ in range(12)]))


@pytest.mark.parametrize("e", ES)
@pytest.mark.parametrize("first", [True, False])
def test_direct_products_match_the_closed_forms(e, first):
    m = X.cosets(e)
    missing = list(range(m // 2)) if first else list(range(m // 2, m))
    which = list(range(m)) if e >= 4 else _sample(e)
    zd, zi = X.factors(missing, which, e)
    for i, c in enumerate(which):
        d, s = X.closed_form(first, c, e)
        assert zd[i] == d and zi[i] * s % R == 1
        assert (d == 0) == (c in missing)
        assert d in (0, 2, R - 2)


@pytest.mark.parametrize("e", [4, 5, 6])
def test_direct_products_match_horner_on_the_coefficients(e):
    m, l = X.cosets(e), 1 << e
    rnd = random.Random(e)
    missing = sorted(rnd.sample(range(m), m // 2 - 3))
    rt = X.roots()
    poly = [1]                                    # prod (y - root), coefficients low to high
    for j in missing:
        root = rt[X.root_index(j, e)]
        poly = [((poly[i - 1] if i else 0) - (poly[i] * root if i < len(poly) else 0)) % R for i in range(len(poly) + 1)]
    assert len(poly) == len(missing) + 1 and poly[-1] == 1

    def horner(y):
        acc = 0
        for coef in reversed(poly):
            acc = (acc * y + coef) % R
        return acc

    which = list(range(m))
    zd, zi = X.factors(missing, which, e)
    for c in which:
        y = pow(pow(X.W, X.brp(l * c, 13), R), l, R)      # x^l at the first position of coset c
        assert y == rt[X.root_index(c, e)]
        assert zd[c] == horner(y)
        assert zi[c] * horner(pow(7, l, R) * y % R) % R == 1


def test_z_is_constant_over_a_coset():
    """x^l is the same at the l positions of a coset, at every e"""
    for e in ES:
        l, m = 1 << e, X.cosets(e)
        for c in (0, 1, m - 1):
            ys = {pow(pow(X.W, X.brp(l * c + k, 13), R), l, R) for k in range(l)}
            assert ys == {X.roots()[X.root_index(c, e)]}


def test_slices_cover_the_list_once():
    for count in (0, 1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 1000, 4095, 4096):
        for p in (1, 2, 4, 8, 16, 32):
            s = X.slices(count, p)
            assert len(s) == p and s[0][0] == 0 and s[-1][1] == count
            assert all(a[1] == b[0] for a, b in zip(s, s[1:]))
            step = -(-count // p)
            assert all(hi - lo <= step for lo, hi in s)


def test_picker_properties():
    for e in ES:
        m = X.cosets(e)
        seen = set()
        for sets in list(range(1, 40)) + [64, 128, 256, 512, 1024]:
            p = X.parts(sets, e)
            seen.add(p)
            assert p & (p - 1) == 0
            if sets * m // 64 >= X.FILL_WAVES:
                assert p == 1
            if p > 1:
                assert (m // 2) // p >= X.MIN_CHAIN            # the longest list still gives every lane a chain
                assert sets * m * (p // 2) // 64 < X.FILL_WAVES   # and half as many lanes would not have filled the chip
        assert seen == set(X.all_parts(e))
    assert X.all_parts(0) == [1, 2, 4, 8] and X.all_parts(6) == [1, 2]
    assert X.parts(512, 6) == 1 and X.parts(8, 0) == 1      # 65,536 lanes are 1,024 waves


def test_plan_on_a_readable_case():
    e, m = 6, 128
    a, b = list(range(64)), list(range(64, 128))
    rows = [a, list(range(63)), b, a, list(range(128)), [], a]
    per_row, chunks = X.plan(rows, e, 3)
    assert per_row == [(0, 0, 0), None, (0, 1, 1), (0, 2, 0), (1, 0, 0), None, (1, 1, 1)]
    assert chunks[0]["runs"] == [(0, 0, 1, 64), (2, 1, 2, 128)]
    assert chunks[1]["runs"] == [(4, 0, 1, 128), (6, 1, 1, 64)]
    assert chunks[1]["missing"][0] == []
    assert chunks[0]["missing"][0] == [64 * X.brp(j, 7) for j in range(64, 128)]
