"""ckzg_hip_verify_coset_kzg_proof_batch_groups without a GPU: the symbol is declared and exported, a settings struct
without GPU state gives C_KZG_ERROR (no CPU fallback), the binding checks its arguments, and the segmented arithmetic of
coset_groups.hip -- replayed on the host over the index maps the product builds (csrc/coset_groups_plan.hpp, through
libhost_shim.so) -- gives, at every coset size and term by term, the integers of tests/coset_groups_expect.py; at e = 6
the replay is byte-equal to hs_cell_groups_replay on the same input.  The expectation helper is checked here by a second
route."""
import ctypes as C
import os
import random
import subprocess

import pytest

import coset_groups_expect as gx
import coset_verify_expect as cx
import rlc_expect as rx
from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, Kzg, KzgError, KZGSettings
from test_abi_exports import declared_symbols

R = gx.R
NAME = "ckzg_hip_verify_coset_kzg_proof_batch_groups"
ES = range(7)


def test_symbol_declared_and_exported():
    assert NAME in declared_symbols()
    assert "    %s;\n" % NAME in open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    assert hasattr(C.CDLL(HIP_SO), NAME)
    hdr = open(os.path.join(ROOT, "include", "ckzg_hip.h")).read()
    assert "#define CKZG_HIP_COSET_GROUPS_CHUNK_ITEMS  16384\n" in hdr
    assert "#define CKZG_HIP_COSET_GROUPS_CHUNK_GROUPS 8192\n" in hdr


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    f = getattr(C.CDLL(HIP_SO), NAME)
    f.restype = C.c_int
    s = KZGSettings()
    ok, st = (C.c_bool * 2)(), (C.c_uint8 * 2)()
    start = (C.c_uint64 * 3)(0, 1, 2)
    idx = (C.c_uint64 * 2)(0, 1)
    for e in ES:
        assert f(ok, st, bytes(96), idx, bytes(64 << e), bytes(96), start, C.c_uint64(2), C.c_uint32(e), C.byref(s)) == 2
    assert f(None, None, None, None, None, None, None, C.c_uint64(0), C.c_uint32(3), C.byref(s)) == 2
    assert f(None, None, None, None, None, None, None, C.c_uint64(0), C.c_uint32(7), C.byref(s)) == 2


def test_binding_checks_its_arguments():
    api = Kzg.__new__(Kzg)   # no library: every check below fails before a call is made
    p48 = bytes(48)
    for e in (0, 3, 6):
        ev = bytes(32 << e)
        for groups in ([([p48], [0], [ev])],                        # not four lists
                       [([p48], [0, 1], [ev], [p48])],              # list lengths
                       [([p48], [0], [ev[:-1]], [p48])],            # short values
                       [([p48], [0], [ev + ev], [p48])],            # the values of another size
                       [([p48[:-1]], [0], [ev], [p48])],            # a short commitment
                       [([p48], [0], [ev], [p48 + b"0"])],          # a long proof
                       [([p48], [-1], [ev], [p48])]):               # an index that is no uint64
            with pytest.raises(KzgError):
                api.verify_coset_kzg_proof_batch_groups(groups, e)
    with pytest.raises(KzgError):
        api.verify_coset_kzg_proof_batch_groups([], -1)
    with pytest.raises(KzgError):
        api.verify_coset_kzg_proof_batch_groups([], 1 << 32)


# ---- the expectation helper, by a second route ----

def _chunk(e, seed, sizes):
    """items with shared and unshared cosets (0, 1 and m - 1 among them), a coset twice in a group, five commitments"""
    rnd = random.Random(seed)
    m, n = 8192 >> e, sum(sizes)
    pick = [0, 1, m - 1, m // 2, 5 % m, 0, m - 1]
    cols = [pick[rnd.randrange(len(pick))] for _ in range(n)]
    item_commit = [rnd.randrange(5) for _ in range(n)]
    values = [[rnd.randrange(R) for _ in range(1 << e)] for _ in range(n)]
    rs = [rnd.randrange(R) for _ in sizes]
    rs[0] = 0
    if len(rs) > 3:
        rs[3] = 1
    return cols, item_commit, values, rs


@pytest.mark.parametrize("e", ES)
def test_expect_interpolation_terms_by_the_rows_route(e):
    sizes = [3, 0, 5, 1, 4]
    cols, item_commit, values, rs = _chunk(e, 1000 + e, sizes)
    l = 1 << e
    src, sc, part_off = gx.group_terms(sizes, item_commit, 5, cols, values, rs, e, 8)
    row_grp, row_col, item_row = gx.rows_of(sizes, cols)
    assert len(row_col) == len({(g, c) for g, c in zip(row_grp, row_col)})
    rows = gx.rows_interp(gx.rows_aggregate(sizes, cols, values, gx.powers(sizes, rs), e), row_col, e)
    per_group = gx.group_interp(rows, row_grp, len(sizes), e)
    first = gx.setup_terms(sizes, item_commit, e, 8)
    for g, n in enumerate(sizes):
        if not n:
            assert first[g] is None
            continue
        t = first[g]
        assert src[t:t + l] == [sum(sizes) + 5 + k for k in range(l)]
        assert sc[t:t + l] == [-v % R for v in per_group[g]]
    # a group of one item: its terms are that item's interpolation polynomial, which takes the item's values on its coset
    a = sum(sizes[:3])
    t = first[3]
    coeffs = [-v % R for v in sc[t:t + l]]
    x = cx.x_of(cols[a], e)
    wl = pow(cx.root_of_unity(8192), 8192 // l, R)
    for j in range(l):
        z = x * pow(wl, cx.brp(j, e), R) % R
        assert sum(ck * pow(z, k, R) for k, ck in enumerate(coeffs)) % R == values[a][j]


# ---- the replay ----

@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    assert hasattr(lib, "hs_coset_groups_replay")
    lib.hs_coset_groups_replay.restype = C.c_long
    lib.hs_cell_groups_replay.restype = C.c_long
    return lib


def _replay(h, sizes, item_commit, num_commits, cols, values, rs, e, quad_max, cap=8192):
    G, n = len(sizes), sum(sizes)
    start = [sum(sizes[:g]) for g in range(G + 1)]
    sc = (C.c_uint32 * (cap * 8))()
    src = (C.c_uint32 * cap)()
    part_off = (C.c_uint32 * (2 * G + 1))()
    info = (C.c_uint32 * 6)()
    total = h.hs_coset_groups_replay(sc, src, part_off, info, C.c_size_t(cap), (C.c_uint64 * (G + 1))(*start), C.c_size_t(G),
                                     (C.c_uint32 * n)(*item_commit), C.c_size_t(num_commits), (C.c_uint64 * n)(*cols),
                                     rx.le32(v for it in values for v in it), rx.le32(rs), rx.le32(gx.roots8193()), C.c_int(e),
                                     C.c_size_t(quad_max))
    return total, sc, src, part_off, info


@pytest.mark.parametrize("e", ES)
def test_host_replay_terms_are_the_integers(h, e):
    """powers of each group's challenge (one is 0, one is 1), the same times x_c^l, the commitment weights and the
    interpolation terms, term by term, with both paddings of the jobs: quad_max_terms on either side of the total"""
    sizes = [3, 0, 5, 1, 4, 9, 2]
    cols, item_commit, values, rs = _chunk(e, 2000 + e, sizes)
    # the terms of all jobs padded to 8 each, before the layout is padded to a multiple of 64: what the rule compares
    total8 = 8 * gx.group_terms(sizes, item_commit, 5, cols, values, rs, e, 8)[2][-1]
    for quad_max, per in ((total8, 8), (total8 - 1, 32)):
        want = gx.group_terms(sizes, item_commit, 5, cols, values, rs, e, per)
        total, sc, src, part_off, info = _replay(h, sizes, item_commit, 5, cols, values, rs, e, quad_max)
        assert total == len(want[0]) and total % 64 == 0 and info[0] == total and info[1] == (1 if per == 8 else 0)
        row_grp, row_col, _ = gx.rows_of(sizes, cols)
        pairs = sum(len(set(item_commit[sum(sizes[:g]):sum(sizes[:g + 1])])) for g in range(len(sizes)))
        assert info[2] == pairs and info[3] == len(row_col)
        rx.check_terms(src[:total], rx.from_le32(sc, total), part_off[:], want)


def test_host_replay_at_64_is_the_cell_replay_byte_for_byte(h):
    sizes = rx.GROUP_SIZES
    G, n = len(sizes), sum(sizes)
    rnd = random.Random(64)
    item_commit = [rnd.randrange(5) for _ in range(n)]
    cols = [(29 * i + 3) % 128 for i in range(n)]
    values = [[rnd.randrange(R) for _ in range(64)] for _ in range(n)]
    rs = rx.group_challenges(641)
    start = [sum(sizes[:g]) for g in range(G + 1)]
    for quad_max in (8192, 0):
        cap = 4096
        total, sc, src, part_off, info = _replay(h, sizes, item_commit, 5, cols, values, rs, 6, quad_max, cap)
        sc2 = (C.c_uint32 * (cap * 8))()
        src2 = (C.c_uint32 * cap)()
        part_off2 = (C.c_uint32 * (2 * G + 1))()
        info2 = (C.c_uint32 * 4)()
        total2 = h.hs_cell_groups_replay(sc2, src2, part_off2, info2, C.c_size_t(cap), (C.c_uint64 * (G + 1))(*start),
                                         C.c_size_t(G), (C.c_uint32 * n)(*item_commit), C.c_size_t(5), (C.c_uint64 * n)(*cols),
                                         rx.le32(v for it in values for v in it), rx.le32(rs), rx.le32(rx.roots_of_unity()),
                                         C.c_size_t(quad_max))
        assert total == total2 > 0
        assert bytes(sc) == bytes(sc2) and bytes(src) == bytes(src2) and bytes(part_off) == bytes(part_off2)
        assert list(info[:4]) == list(info2)


def test_host_replay_refuses_what_does_not_fit(h):
    sizes = [2, 2]
    cols, item_commit, values, rs = _chunk(2, 5, sizes)
    assert _replay(h, sizes, item_commit, 5, cols, values, rs, 2, 8192, cap=64)[0] == 64
    assert _replay(h, sizes, item_commit, 5, cols, values, rs, 2, 0, cap=64)[0] == -1    # 32-term jobs: 128 terms
    assert _replay(h, sizes, item_commit, 5, cols, values, rs, 7, 8192)[0] == -2


def test_launch_pickers(h):
    """the parts rules of coset_groups_plan.hpp: 70 items on one coset and 1 item give 16 parts by the rule of
    coset_verify_agg_parts with the rows in the place of the cosets; the per-group sum splits when a group has many rows"""
    e = 2
    sizes = [70, 1]
    cols = [3] * 70 + [4]
    values = [[1] * 4 for _ in range(71)]
    info = _replay(h, sizes, [0] * 71, 1, cols, values, [2, 3], e, 8192)[4]
    assert info[3] == 2 and info[4] == 16
    sizes = [80, 1]
    cols = list(range(80)) + [0]
    info = _replay(h, sizes, [0] * 81, 1, cols, [[1] * 4 for _ in range(81)], [2, 3], e, 8192)[4]
    assert info[3] == 81 and info[4] == 1 and info[5] == 2   # 81 rows over 2 groups: more than 32 rows a lane at one part
