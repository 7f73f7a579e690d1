"""The host half of ckzg_hip_verify_kzg_proof_batch_locate / ckzg_hip_verify_blob_kzg_proof_batch_locate without a GPU
(csrc/locate_plan.hpp through libhost_shim.so): the bisection over a synthetic predicate -- verdicts, the number of
checks as a property of the rules, the hand-over -- and the whole second half in host arithmetic (P1, the r^i scaling,
prefix sums, the range predicate with the real pairing) over every well-formed verify_kzg_proof consensus vector."""
import ctypes as C
import hashlib
import itertools
import os
import random
import subprocess

import pytest

from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, KZGSettings, TRUSTED_SETUP
from test_abi_exports import declared_symbols
from test_gpu_point_proofs import _spec_items

NAMES = ("ckzg_hip_g1_prefix_sums", "ckzg_hip_verify_kzg_proof_batch_locate", "ckzg_hip_verify_blob_kzg_proof_batch_locate")


@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    assert hasattr(lib, "hs_locate_bisect") and hasattr(lib, "hs_locate_points_host")
    lib.hs_locate_bisect.restype = None
    lib.hs_locate_points_host.restype = None
    return lib


def test_symbols_declared_and_exported():
    exports = open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    lib = C.CDLL(HIP_SO)
    for name in NAMES:
        assert name in declared_symbols()
        assert "    %s;\n" % name in exports
        assert hasattr(lib, name)


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    lib = C.CDLL(HIP_SO)
    s = KZGSettings()
    ok, st, stats = (C.c_bool * 2)(), (C.c_uint8 * 2)(), (C.c_uint64 * 3)()
    f = lib.ckzg_hip_verify_kzg_proof_batch_locate
    f.restype = C.c_int
    assert f(ok, st, stats, bytes(96), bytes(64), bytes(64), bytes(96), C.c_uint64(2), C.byref(s)) == 2
    g = lib.ckzg_hip_verify_blob_kzg_proof_batch_locate
    g.restype = C.c_int
    assert g(ok, st, stats, bytes(2 * 131072), bytes(96), bytes(96), C.c_uint64(2), C.byref(s)) == 2
    p = lib.ckzg_hip_g1_prefix_sums
    p.restype = C.c_int
    out = C.create_string_buffer(2 * 144)
    assert p(out, bytes(2 * 144), C.c_uint64(2), C.byref(s)) == 2


def test_option_is_validated():
    f = C.CDLL(HIP_SO).ckzg_hip_set_option
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_int64]
    assert f(b"locate_max_checks", -1) == 1


# ---- the bisection over the predicate "no bad item in the range" ----

def _bisect(h, bad, invalid, max_checks=-1):
    n = len(bad)
    ok, opn, stats = (C.c_uint8 * max(n, 1))(), (C.c_uint8 * max(n, 1))(), (C.c_uint64 * 2)()
    h.hs_locate_bisect(ok, stats, opn, bytes(bad), bytes(invalid), C.c_uint64(n), C.c_int64(max_checks))
    return [bool(v) for v in ok[:n]], [bool(v) for v in opn[:n]], stats[0], stats[1]


def _ceil_log2(m):
    return (m - 1).bit_length()


def _check_full(h, bad, invalid):
    n = len(bad)
    ok, opn, checks, nopen = _bisect(h, bad, invalid)
    false_items = sum(1 for b, i in zip(bad, invalid) if b and not i)
    assert ok == [not b and not i for b, i in zip(bad, invalid)], (bad, invalid)
    assert not any(opn) and nopen == 0
    if all(invalid):
        assert checks == 0
    elif false_items == 0:
        assert checks == 1
    else:
        assert 1 <= checks <= 1 + 2 * false_items * _ceil_log2(n), (bad, invalid, checks)
    return checks


def test_every_mask_up_to_ten_items(h):
    for n in range(1, 11):
        for mask in itertools.product((0, 1), repeat=n):
            _check_full(h, mask, [0] * n)
    # with invalid items: every mask of bad items against several masks of invalid ones (an invalid item is inert
    # whatever its bad byte says)
    rnd = random.Random(1)
    for n in range(1, 11):
        inv_masks = {tuple([1] * n), tuple(1 if i == 0 else 0 for i in range(n)), tuple(1 if i == n - 1 else 0 for i in range(n))}
        for _ in range(3):
            inv_masks.add(tuple(rnd.randrange(2) for _ in range(n)))
        for inv in inv_masks:
            for mask in itertools.product((0, 1), repeat=n):
                _check_full(h, mask, inv)


def test_one_false_item_costs_at_most_two_checks_per_level(h):
    for n in (2, 3, 257, 1000):
        for pos in {0, 1, n // 2 - 1, n // 2, n - 2, n - 1}:
            bad = [0] * n
            bad[pos] = 1
            assert _check_full(h, bad, [0] * n) <= 1 + 2 * _ceil_log2(n)


def test_random_masks_up_to_a_thousand_items(h):
    rnd = random.Random(2)
    for nbad in (1, 2, 10):
        for _ in range(40):
            n = rnd.randrange(nbad, 1001)
            bad = [0] * n
            for i in rnd.sample(range(n), nbad):
                bad[i] = 1
            invalid = [1 if rnd.randrange(50) == 0 else 0 for _ in range(n)]
            _check_full(h, bad, invalid)


def _expected_open(bad, invalid, max_checks):
    """the rules of locate_plan.hpp replayed in Python: (ok, open flags, checks)"""
    n = len(bad)
    fine = lambda a, b: not any(bad[i] and not invalid[i] for i in range(a, b))
    ok, opn = [False] * n, [False] * n
    if all(invalid):
        return ok, opn, 0
    checks = 1
    if fine(0, n):
        return [not i for i in invalid], opn, 1
    level = [(0, n)] if n > 1 else []
    while level:
        if checks + 2 * len(level) > max_checks:
            for a, b in level:
                for i in range(a, b):
                    opn[i] = True
            break
        nxt = []
        for a, b in level:
            mid = a + (b - a + 1) // 2
            checks += 1
            left = fine(a, mid)
            if left:
                right = False
            else:
                checks += 1
                right = fine(mid, b)
            for (x, y), good in (((a, mid), left), ((mid, b), right)):
                if good:
                    for i in range(x, y):
                        ok[i] = not invalid[i]
                elif y - x > 1:
                    nxt.append((x, y))
        level = nxt
    return ok, opn, checks


@pytest.mark.parametrize("max_checks", [0, 5])
def test_hand_over(h, max_checks):
    rnd = random.Random(3 + max_checks)
    cases = [([1] * 8, [0] * 8), ([0] * 7 + [1], [0] * 8), ([1], [0]), ([0, 1], [0, 0])]
    for _ in range(200):
        n = rnd.randrange(1, 300)
        bad = [1 if rnd.randrange(n) < rnd.choice((1, 2, 10)) else 0 for _ in range(n)]
        invalid = [1 if rnd.randrange(40) == 0 else 0 for _ in range(n)]
        cases.append((bad, invalid))
    handed = 0
    for bad, invalid in cases:
        ok, opn, checks, nopen = _bisect(h, bad, invalid, max_checks)
        want_ok, want_open, want_checks = _expected_open(bad, invalid, max_checks)
        assert checks <= max(max_checks, 1) and checks == want_checks   # (0: only the root)
        assert opn == want_open and (nopen > 0) == any(opn)               # exactly the unsplit false ranges
        handed += 1 if any(opn) else 0
        for i in range(len(bad)):
            if not opn[i]:   # every item outside them is already right
                assert ok[i] == (not bad[i] and not invalid[i])
            else:
                assert ok[i] is False
        if any(opn):
            assert any(bad[i] and not invalid[i] and opn[i] for i in range(len(bad)))   # an open range is a false one
    assert handed > 20


# ---- the second half on the host, with the real pairing ----

def _g2(h, b96):
    aff = C.create_string_buffer(192)
    assert h.hs_g2_uncompress(aff, b96) == 0
    gen = C.create_string_buffer(288)
    h.hs_g2_generator(gen)
    return aff.raw + gen.raw[192:]


def _points_host(h, items, max_checks=-1):
    n = len(items)
    lines = open(TRUSTED_SETUP).read().split()
    assert lines[0] == "4096" and lines[1] == "65"
    tau = _g2(h, bytes.fromhex(lines[2 + 4096 + 1]))
    ok, st, stats, r32 = (C.c_uint8 * n)(), (C.c_uint8 * n)(), (C.c_uint64 * 2)(), C.create_string_buffer(32)
    j = lambda k: b"".join(t[k] for t in items)
    h.hs_locate_points_host(ok, st, stats, r32, j(0), j(1), j(2), j(3), C.c_uint64(n), tau, C.c_int64(max_checks))
    return [bool(v) for v in ok], list(st), stats[0], r32.raw


def test_all_spec_vectors_on_the_host(h):
    items = _spec_items()
    assert len(items) >= 100 and {t[4] for t in items} == {True, False, None}
    ok, st, checks, r32 = _points_host(h, items)
    for i, it in enumerate(items):
        if it[4] is None:
            assert st[i] == 1 and ok[i] is False, (i, it[5])
        else:
            assert st[i] == 0 and ok[i] is it[4], (i, it[5], ok[i])
    nfalse = sum(1 for t in items if t[4] is False)
    assert 1 < checks <= 1 + 2 * nfalse * _ceil_log2(len(items))
    # the chunk's challenge is the digest of the library's batch transcript over the items as given
    d = hashlib.sha256(b"RCKZGBATCH___V1_" + (4096).to_bytes(8, "big") + len(items).to_bytes(8, "big"))
    for c, z, y, p in (t[:4] for t in items):
        d.update(c + z + y + p)
    assert r32 == d.digest()


def test_true_vectors_alone_cost_one_check(h):
    items = [t for t in _spec_items() if t[4] is True]
    inv = [t for t in _spec_items() if t[4] is None][:2]
    ok, st, checks, _ = _points_host(h, items)
    assert ok == [True] * len(items) and st == [0] * len(items) and checks == 1
    # an invalid item in a good batch is settled from its flag: still one check
    mixed = items[:5] + inv[:1] + items[5:] + inv[1:]
    ok, st, checks, _ = _points_host(h, mixed)
    assert checks == 1 and ok == [t[4] is True for t in mixed] and st == [1 if t[4] is None else 0 for t in mixed]
