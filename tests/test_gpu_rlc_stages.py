"""The weights of the batch checks and the rows of the batch transcript, read off the device and compared with
integers.  A weight is the one value a verdict cannot check: for an honest batch any weights pass, for a spoilt one
almost any weights fail, so r^(i mod 256), weights that restart somewhere, r = 1 or a transcript row that never holds
y leave every verdict of the suite as it was and only cost soundness.  tests/native/stage_shim.hip (libstage_shim.so:
its entry file linked with the product's own object files, so the kernels are the product's binary code) runs each
stage on chosen inputs and returns its whole output buffer:

    rpow_at (rpow2.hpp)                               every table entry: indices 2^k - 1, 2^k, 2^k + 1, k < 24
    rlc_scalars_enqueue                               k_rlc_scalars
    coset_rlc_scalars_enqueue at cosets of 64         k_coset_rlc_scalars, k_coset_commit_weights (a cell batch's)
    coset_group_rlc_scalars_enqueue at cosets of 64   k_coset_group_rlc_scalars, k_group_commit_weights (cell groups')
    blob_group_scalars_enqueue                        k_blob_group_scalars, k_blob_group_ysum
    locate_scale_enqueue                              k_locate_scale
    batch_transcript_rows_device                      k_batch_transcript_rows

Every comparison is exact: Python integers (tests/rlc_expect.py) for scalars and bytes, the CPU oracle's scalar
multiplication for points.  Challenges: 0, 1, 2, R - 1 and two random values everywhere; the grouped stages get one
value per group, 0 and 1 among them.

After any non-zero return of a shim call (a HIP error or the shim's 20 s deadline) every later test of the module
fails at once without launching anything."""
import ctypes as C
import os
import random
import subprocess

import pytest

import rlc_expect as rx
from rlc_expect import R
from conftest import ORACLE_SO, ROOT, SHIM_SO
from test_gpu_dev_arith import Group, INF

pytestmark = pytest.mark.gpu

# CKZG_STAGE_SHIM_SO: another build of the shim (the way conftest.py takes CKZG_HIP_SO / CKZG_SHIM_SO)
STAGE_SHIM_SO = os.path.abspath(os.environ["CKZG_STAGE_SHIM_SO"]) if os.environ.get("CKZG_STAGE_SHIM_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "libstage_shim.so")
# every exported function this module binds (tests/test_stage_shim_cpu.py checks the library for them)
STAGE_FUNCTIONS = ["ss_rpow_at", "ss_rlc_scalars", "ss_cell_rlc_scalars", "ss_cell_groups_scalars", "ss_blob_groups_scalars",
                   "ss_locate_scale", "ss_batch_transcript_rows"]
CHALLENGES = rx.challenges(0x51a9e)
CAP_TERMS = 4096


class StageShim:
    """libstage_shim.so; remembers the first failed call and refuses every later one"""

    def __init__(self, lib):
        self.lib = lib
        self.dead = None

    def call(self, name, *args):
        if self.dead is not None:
            pytest.fail("an earlier shim call (%s) returned %d: nothing is launched any more" % self.dead)
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            self.dead = (name, rc)
            pytest.fail("%s returned %d" % (name, rc))


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(STAGE_SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libstage_shim.so"])
    lib = C.CDLL(STAGE_SHIM_SO)
    for fn in STAGE_FUNCTIONS:
        getattr(lib, fn).restype = C.c_int
    return StageShim(lib)


@pytest.fixture(scope="module")
def roots():
    return rx.roots_of_unity()


@pytest.fixture(scope="module")
def roots_raw(roots):
    return rx.le32(roots)


@pytest.fixture(scope="module")
def grp():
    pkg = os.path.join(ROOT, "c-kzg-4844_amd")
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", pkg, "csrc/libhost_shim.so"])
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    o, h = C.CDLL(ORACLE_SO), C.CDLL(SHIM_SO)
    for fn in ("og1_equal", "og1_is_inf", "og1_in_subgroup"):
        getattr(o, fn).restype = C.c_bool
    return Group(o, h)


def _scalars(rnd, n):
    """n values with 0, R - 1 and 1 among them (from n = 3 on), the rest random"""
    vals = [rnd.randrange(R) for _ in range(n)]
    for at, v in ((n // 2, 0), (n - 1, R - 1), (0, 1)):
        if n >= 3:
            vals[at] = v
    return vals


# ---- 1. rpow_at ----

RPOW_INDICES = sorted({0, 1, 2, 3, (1 << 24) - 1} | {(1 << k) + d for k in range(24) for d in (-1, 0, 1) if 0 <= (1 << k) + d < 1 << 24})


@pytest.mark.parametrize("r", CHALLENGES)
def test_rpow_at_reaches_every_table_entry(shim, r):
    assert RPOW_INDICES[-1] == (1 << 24) - 1 and (1 << 23) + 1 in RPOW_INDICES
    n = len(RPOW_INDICES)
    out = C.create_string_buffer(32 * n)
    shim.call("ss_rpow_at", out, rx.le32([r]), (C.c_uint32 * n)(*RPOW_INDICES), n)
    got = rx.from_le32(out, n)
    for i, g in zip(RPOW_INDICES, got):
        assert g == pow(r, i, R), "r^%d" % i


# ---- 2. rlc_scalars_enqueue ----

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 65539])
def test_rlc_scalars(shim, n):
    rnd = random.Random(n)
    z = _scalars(rnd, n)
    z_raw = rx.le32(z)
    for r in CHALLENGES:
        sc = C.create_string_buffer(b"\xa5" * (6 * n * 32), 6 * n * 32)   # the stage clears the vector itself
        shim.call("ss_rlc_scalars", sc, z_raw, rx.le32([r]), C.c_size_t(n))
        got = rx.from_le32(sc, 6 * n)
        want = [0] * (6 * n)
        pw = 1
        for i in range(n):
            want[0 * 2 * n + n + i] = pw                # r^i on proof i
            want[1 * 2 * n + n + i] = pw * z[i] % R     # r^i z_i on proof i
            want[2 * 2 * n + i] = pw                    # r^i on commitment i
            pw = pw * r % R
        if got != want:
            at = next(t for t in range(6 * n) if got[t] != want[t])
            pytest.fail("r = %x, n = %d: scalar %d of vector %d is %x, expected %x" % (r, n, at % (2 * n), at // (2 * n), got[at], want[at]))


# ---- 3. the scalars of a cell batch: coset_rlc_scalars_enqueue at cosets of 64 ----

def _member_lists(rnd, n):
    """the cells dealt to commitments with member lists of 1, 63, 64, 65 and 107 cells (n = 300; whatever fits
    below that), each list in shuffled order"""
    cells = list(range(n))
    rnd.shuffle(cells)
    lists, at = [], 0
    for size in (1, 63, 64, 65, 107):
        if at >= n:
            break
        lists.append(cells[at:at + size])
        at += size
    if at < n:
        lists.append(cells[at:])
    return lists


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_cell_rlc_scalars(shim, roots, roots_raw, n):
    rnd = random.Random(7000 + n)
    cols = [(37 * i + 5) % 128 for i in range(n)]       # every one of the 128 columns at n = 300
    assert n < 300 or set(cols) == set(range(128))
    lists = _member_lists(rnd, n)
    assert n < 300 or [len(m) for m in lists] == [1, 63, 64, 65, 107]
    nc = len(lists)
    start = [0]
    for m in lists:
        start.append(start[-1] + len(m))
    members = [i for m in lists for i in m]
    assert sorted(members) == list(range(n))
    for r in CHALLENGES:
        rp, vrp, vwrp = (C.create_string_buffer(32 * n) for _ in range(3))
        vw = C.create_string_buffer(32 * nc)
        shim.call("ss_cell_rlc_scalars", rp, vrp, vwrp, vw, (C.c_uint32 * n)(*cols), (C.c_uint32 * (nc + 1))(*start),
                  (C.c_uint32 * n)(*members), rx.le32([r]), roots_raw, C.c_size_t(n), C.c_size_t(nc))
        pw = [pow(r, i, R) for i in range(n)]
        assert rx.from_le32(rp, n) == pw, "d_rp, r = %x" % r
        assert rx.from_le32(vrp, n) == pw, "vec_rp, r = %x" % r
        assert rx.from_le32(vwrp, n) == [pw[i] * roots[64 * rx.brev7(cols[i])] % R for i in range(n)], "vec_wrp, r = %x" % r
        assert rx.from_le32(vw, nc) == [sum(pw[i] for i in m) % R for m in lists], "commitment weights, r = %x" % r


# ---- 4. the grouped stages ----

@pytest.mark.parametrize("quad_max", [8192, 0])   # both paddings of the jobs: 8 terms per partial and 32
def test_blob_group_scalars(shim, quad_max):
    sizes = rx.GROUP_SIZES
    G, N = len(sizes), sum(sizes)
    rnd = random.Random(4100 + quad_max)
    z, y = _scalars(rnd, N), _scalars(rnd, N)[::-1]
    rs = rx.group_challenges(4200 + quad_max)
    assert rs[2] == 0 and rs[5] == 1
    start = [sum(sizes[:g]) for g in range(G + 1)]
    per = 8 if quad_max else 32
    sc = C.create_string_buffer(32 * CAP_TERMS)
    ry = C.create_string_buffer(32 * N)
    src = (C.c_uint32 * CAP_TERMS)()
    part_off = (C.c_uint32 * (2 * G + 1))()
    info = (C.c_uint32 * 2)()
    shim.call("ss_blob_groups_scalars", sc, ry, src, part_off, info, C.c_size_t(CAP_TERMS), (C.c_uint64 * (G + 1))(*start),
              C.c_size_t(G), rx.le32(z), rx.le32(y), rx.le32(rs), C.c_size_t(quad_max))
    total = info[0]
    assert info[1] == (1 if quad_max else 0) and total % 64 == 0
    want = rx.blob_group_terms(sizes, z, y, rs, per)
    assert total == len(want[0])
    rx.check_terms(src[:total], rx.from_le32(sc, total), part_off[:], want)
    want_ry = [pow(rs[g], i, R) * y[start[g] + i] % R for g in range(G) for i in range(sizes[g])]
    assert rx.from_le32(ry, N) == want_ry


@pytest.mark.parametrize("quad_max", [8192, 0])
def test_cell_group_scalars(shim, roots, roots_raw, quad_max):
    sizes = rx.GROUP_SIZES
    G, N = len(sizes), sum(sizes)
    rnd = random.Random(4300 + quad_max)
    num_commits = 5
    cell_commit = [rnd.randrange(num_commits) for _ in range(N)]
    cols = [(29 * i + 3) % 128 for i in range(N)]
    assert set(cols) == set(range(128))
    rs = rx.group_challenges(4400 + quad_max)
    start = [sum(sizes[:g]) for g in range(G + 1)]
    per = 8 if quad_max else 32
    sc = C.create_string_buffer(32 * CAP_TERMS)
    rp = C.create_string_buffer(32 * N)
    src = (C.c_uint32 * CAP_TERMS)()
    part_off = (C.c_uint32 * (2 * G + 1))()
    info = (C.c_uint32 * 4)()
    shim.call("ss_cell_groups_scalars", sc, rp, src, part_off, info, C.c_size_t(CAP_TERMS), (C.c_uint64 * (G + 1))(*start),
              C.c_size_t(G), (C.c_uint32 * N)(*cell_commit), C.c_size_t(num_commits), (C.c_uint64 * N)(*cols), rx.le32(rs),
              roots_raw, C.c_size_t(quad_max))
    total = info[0]
    assert info[1] == (1 if quad_max else 0) and total % 64 == 0
    want = rx.cell_group_terms(sizes, cell_commit, num_commits, cols, rs, roots, per)
    assert total == len(want[0])
    # the 64 terms of the interpolation commitment belong to a later stage: this one leaves them zero
    rx.check_terms(src[:total], rx.from_le32(sc, total), part_off[:], want, unpinned=0)
    assert rx.from_le32(rp, N) == [pow(rs[g], i, R) for g in range(G) for i in range(sizes[g])]


# ---- 5. locate_scale_enqueue ----

@pytest.fixture(scope="module")
def locate_points(grp):
    """300 items (P1_i, -proof_i), affine; items 7 and 64 are the infinity pair of an invalid item"""
    rnd = random.Random(5150)
    base = [grp.affine(grp.rand(rnd)) for _ in range(12)]
    p1 = [base[(5 * i + 1) % 12] for i in range(300)]
    negp = [base[(7 * i + 3) % 12] for i in range(300)]
    for i in (7, 64):
        p1[i] = negp[i] = INF
    return p1, negp


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_locate_scale(shim, grp, locate_points, n):
    p1, negp = locate_points[0][:n], locate_points[1][:n]
    for r in CHALLENGES:
        ab = C.create_string_buffer(144 * 2 * n)
        shim.call("ss_locate_scale", ab, b"".join(p1), b"".join(negp), rx.le32([r]), C.c_size_t(n))
        raw = ab.raw
        memo = {}
        for i in range(n):
            k = pow(r, i, R)
            for half, pt in ((0, p1[i]), (1, grp.neg(negp[i]) if negp[i] != INF else INF)):
                got = raw[144 * (half * n + i):144 * (half * n + i + 1)]
                if k == 0 or pt == INF:
                    assert grp.is_inf(got), (r, i, half)
                    continue
                if (pt, k) not in memo:
                    memo[(pt, k)] = grp.mul(pt, k)
                assert not grp.is_inf(got) and grp.equal(got, memo[(pt, k)]), "r = %x: %s_%d" % (r, "AB"[half], i)
        if r == 0:
            assert all(grp.is_inf(raw[144 * t:144 * t + 144]) for t in list(range(1, n)) + list(range(n + 1, 2 * n)))


# ---- 6. batch_transcript_rows_device ----

@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_transcript_rows(shim, n):
    rnd = random.Random(6000 + n)
    z = _scalars(rnd, n)
    y = [(v + 1 + rnd.randrange(R - 2)) % R for v in z]       # z_i != y_i throughout
    if n >= 3:
        y[0], y[1] = 0, R - 1
    if n == 1:
        z, y = [R - 1], [0]
    assert all(a != b for a, b in zip(z, y))
    pts = bytes(rnd.randrange(256) for _ in range(2 * n * 48))   # copied as they are: any bytes
    rows = C.create_string_buffer(160 * n)
    shim.call("ss_batch_transcript_rows", rows, pts, rx.le32(z), rx.le32(y), C.c_size_t(n))
    for i in range(n):
        want = pts[48 * i:48 * i + 48] + z[i].to_bytes(32, "big") + y[i].to_bytes(32, "big") + pts[48 * (n + i):48 * (n + i) + 48]
        assert rows.raw[160 * i:160 * i + 160] == want, "row %d" % i
