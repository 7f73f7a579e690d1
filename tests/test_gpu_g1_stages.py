"""The stages that add up G1 points, read off the device and compared with integers.  The entry points reach them
with the trusted setup as bases, with honest points and at the launch shapes the product's sizes happen to select; here
the bases are a_i * G with chosen a_i, the digit vectors and job layouts are the test's, and every expected value is one
integer mod r (tests/g1_expect.py; each reference has a second route in tests/test_g1_expect_cpu.py).
tests/native/g1_shim.hip (libg1_shim.so: its entry file linked with the product's own object files, so the kernels are
the product's binary code) runs each stage and returns its whole output buffer:

    build_fixed_base_table                 k_window_bases_quad, k_batch_to_affine (to392), k_table_seeds, k_table_steps<8>
    msm_from_digits_device                 k_msm_accumulate<256, RAW>, msm_sum_pairs, xyzz28_madd_alt's doubling and
                                           cancellation branches, block_reduce_xyzz28_quad, and the folds of run_msm:
                                           k_msm_fold_finalize (A), k_msm_reduce_partials + k_msm_finalize (B),
                                           k_msm_finalize_tree<2|4|8>, the chain in k_msm_finalize
    msm_small_vectors_device               k_msm_small<64 | 16 | 8>
    commit_blobs_enqueue, msm_commit_table_raw_device      k_blob_digits, k_raw_digits (the recoding, as a property)
    call_table_enqueue + table_sums_enqueue                the X28 table, k_raw_digits_n, k_msm_accumulate_x28
    batch_to_affine_device                 run lengths 1, 4, 16, 128
    lincomb_multi_device, bucket_msm_enqueue, g1_prefix_scan_enqueue      several jobs / segments

Exact everywhere: bytes for table entries, affine and compressed points, digits and status; points for XYZZ outputs
(x / zz, y / zzz, zzz^2 = zz^3, infinity as the product encodes it); the guard behind every output intact.  The launch
shapes are asserted through gs_msm_plan (what pick_pairs_per_block(_fixed) returns), not trusted from a table.

Out of reach here: table segments longer than 16 entries (k_table_steps with seg > 16 needs a table of gigabytes; the
end-to-end tests build those), and the G1 transforms of fk20.hip, whose launch forms the batch-size tests span.

After any non-zero return of a shim call (a HIP error or the shim's 20 s deadline) every later test of the module
fails at once without launching anything."""
import array
import ctypes as C
import os
import random
import subprocess

import pytest

import g1_expect as gx
from g1_expect import R, LAMBDA, Shape
from conftest import ROOT, ORACLE_SO

pytestmark = pytest.mark.gpu

# CKZG_G1_SHIM_SO: another build of the shim (the way conftest.py takes CKZG_HIP_SO / CKZG_SHIM_SO)
G1_SHIM_SO = os.path.abspath(os.environ["CKZG_G1_SHIM_SO"]) if os.environ.get("CKZG_G1_SHIM_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "libg1_shim.so")
# every exported function this module binds (tests/test_g1_expect_cpu.py checks the library for them)
G1_FUNCTIONS = ["gs_msm_plan", "gs_build_table", "gs_msm_from_digits", "gs_msm_small", "gs_commit_blobs", "gs_commit_raw",
                "gs_table_sums", "gs_batch_to_affine", "gs_lincomb_multi", "gs_bucket_msm", "gs_prefix_scan"]
SZ = C.c_size_t
GUARD = 0xa5


class G1Shim:
    """libg1_shim.so; remembers the first failed call and refuses every later one"""

    def __init__(self, lib):
        self.lib = lib
        self.dead = None

    def call(self, name, *args):
        """the stage's own return value (a refusal is a result); the call's return must be 0"""
        if self.dead is not None:
            pytest.fail("an earlier shim call (%s) returned %d: nothing is launched any more" % self.dead)
        rc = C.c_int(-1)
        run = getattr(self.lib, name)(*args, C.byref(rc))
        if run != 0:
            self.dead = (name, run)
            pytest.fail("%s returned %d" % (name, run))
        return rc.value

    def plan(self, npoints, wbits, nvec, fixed=1):
        ppb, bpv = C.c_uint32(0), C.c_uint32(0)
        assert self.lib.gs_msm_plan(npoints, wbits, SZ(nvec), fixed, C.byref(ppb), C.byref(bpv)) == 0
        return ppb.value, bpv.value


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(G1_SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libg1_shim.so"])
    lib = C.CDLL(G1_SHIM_SO)
    for fn in G1_FUNCTIONS:
        getattr(lib, fn).restype = C.c_int
    return G1Shim(lib)


@pytest.fixture(scope="module")
def src():
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    return gx.G1Source(C.CDLL(ORACLE_SO))


def guarded(nbytes, guard):
    """a buffer of nbytes + guard bytes, all of them the pattern"""
    return C.create_string_buffer(bytes([GUARD]) * (nbytes + guard), nbytes + guard)


def guard_intact(buf, nbytes, what):
    assert buf.raw[nbytes:] == bytes([GUARD]) * (len(buf) - nbytes), "%s: the guard behind the output was written" % what


def pack(d):
    return array.array("h", d).tobytes()


def unpack(b):
    a = array.array("h")
    a.frombytes(b)
    return a


def run_form(ppb, bpv, nvec):
    """run_msm's choice among its folds"""
    if 8 < bpv <= 512 and ppb <= 1024 and nvec * bpv <= 512:
        return "A"
    if bpv > 8:
        return "B"
    if bpv >= 2 and nvec <= 4096:
        return "tree2" if bpv <= 2 else ("tree4" if bpv <= 4 else "tree8")
    return "chain"


def special_bases(n, rnd, ends=True):
    """random a_i with, where n allows: infinity first, last and in the middle (ends = False: second and last but one,
    so that the first and the last pair of a digit vector select finite entries), a repeated base, P and -P, 1, r - 1"""
    a = [rnd.randrange(1, R) for _ in range(n)]
    if n >= 3 and ends:
        a[0] = a[n - 1] = 0
    if n >= 16 and not ends:
        a[2] = a[n - 2] = 0
    if n >= 5:
        a[n // 2] = 0
        a[1], a[3] = 1, R - 1
    if n >= 16:
        a[5] = a[4]
        a[7] = R - a[6]
        a[9] = a[4]
    return a


def bases_raw(src, a):
    return b"".join(src.raw(v) for v in a)


def device_table(shim, src, a, c):
    n = len(a)
    nbytes = gx.twin_for(c) * n * (1 << (c - 1)) * 96
    buf = guarded(nbytes, 96 * 4)
    assert shim.call("gs_build_table", buf, SZ(len(buf)), bases_raw(src, a), n, c) == 0
    guard_intact(buf, nbytes, "table (%d, %d)" % (n, c))
    return buf.raw[:nbytes]


def from_digits(shim, table, n, c, vecs, order):
    """the compressed sums of the vectors vecs[order[v]]"""
    packed = [pack(v) for v in vecs]
    nvec = len(order)
    out = guarded(48 * nvec, 96)
    assert shim.call("gs_msm_from_digits", out, SZ(len(out)), table, SZ(len(table)), n, c, b"".join(packed[j] for j in order), SZ(nvec)) == 0
    guard_intact(out, 48 * nvec, "sums")
    return [out.raw[48 * v:48 * v + 48] for v in range(nvec)]


def check_sums(got, want, order, what):
    for v, j in enumerate(order):
        assert got[v] == want[j], "%s: vector %d (kind %d) is %s, expected %s" % (what, v, j, got[v].hex(), want[j].hex())


def digit_kinds(n, c, rnd):
    """seven digit vectors: random, all zero, one non-zero digit at the first and at the last pair, +-2^(c-1)
    everywhere, an empty k2 half, an empty k1 half, random"""
    half, twin = 1 << (c - 1), gx.twin_for(c)
    pairs, phi = 2 * twin * n, twin * n
    rand = lambda: [rnd.randint(-half, half) for _ in range(pairs)]
    ends = [0] * pairs
    ends[0], ends[-1] = 3 % (half + 1) or 1, -half
    k1_only, k2_only = rand(), rand()
    k1_only[:phi] = [0] * phi
    k2_only[phi:] = [0] * phi
    return [rand(), [0] * pairs, ends, [rnd.choice((-half, half)) for _ in range(pairs)], k1_only, k2_only, rand()]


def period7(nvec):
    """an order whose period is coprime to 8, 16, 32 and 64"""
    return [(3 * v) % 7 for v in range(nvec)]


# ---- 1. tables ----

TABLE_SHAPES = [(1, 2), (3, 4), (5, 6), (67, 5), (256, 4)]


@pytest.mark.parametrize("npoints,wbits", TABLE_SHAPES)
def test_fixed_base_table_is_every_multiple(shim, src, npoints, wbits):
    """the whole table, bytewise; half < 16 (one segment is the chain) and half = 32 (two segments of 16); the chain
    count is no multiple of 8 at 3, 5 and 67 points; infinity first, last and in the middle, a repeated base, P and
    -P, a = 1, a = r - 1"""
    a = special_bases(npoints, random.Random(npoints * 100 + wbits))
    if npoints == 3:
        a = [0, 1, R - 1]
    got = device_table(shim, src, a, wbits)
    want = gx.table_raw(src, a, wbits)
    assert len(got) == len(want)
    if got != want:
        at = next(i for i in range(0, len(want), 96) if got[i:i + 96] != want[i:i + 96]) // 96
        half = 1 << (wbits - 1)
        pytest.fail("entry %d (chain %d, e = %d) is %s, expected %s" % (at, at // half, at % half, got[96 * at:96 * at + 96].hex(), want[96 * at:96 * at + 96].hex()))


def test_the_table_shapes_reach_both_segment_layouts():
    halves = {1 << (c - 1) for _, c in TABLE_SHAPES}
    assert any(h < 16 for h in halves) and 32 in halves   # seg = half, and two segments of 16
    assert {(gx.twin_for(c) * n) % 8 != 0 for n, c in TABLE_SHAPES} == {True, False}


# ---- 2. sums from digits, random digits ----

# (npoints, wbits, nvec): the launch forms are asserted below, through gs_msm_plan
DIGIT_CASES = [(256, 4, 1), (256, 4, 9), (256, 4, 33), (256, 4, 64), (256, 4, 65), (256, 4, 513), (256, 4, 1024), (256, 4, 4097),
               (64, 4, 200), (64, 5, 1), (100, 4, 1)]
_tables = {}


def shared_table(shim, src, n, c):
    """one table (and one set of bases) per shape for the random-digit cases"""
    if (n, c) not in _tables:
        rnd = random.Random(n * 1000 + c)
        a = special_bases(n, rnd, ends=False)
        _tables[(n, c)] = (a, device_table(shim, src, a, c), digit_kinds(n, c, rnd))
    return _tables[(n, c)]


def test_the_digit_cases_reach_every_launch_form(shim):
    """form A with even and odd bpv, form B, the three trees, the chain with bpv 1 and 2, the phi boundary on a block
    edge and inside a block, a ragged last block: a case list that stops reaching one of them fails here"""
    seen, phi_edge, phi_inside, ragged = set(), False, False, False
    for n, c, nvec in DIGIT_CASES:
        ppb, bpv = shim.plan(n, c, nvec)
        pairs = 2 * gx.twin_for(c) * n
        assert bpv == (pairs + ppb - 1) // ppb
        form = run_form(ppb, bpv, nvec)
        seen.add((form, bpv % 2 if form == "A" else (bpv if form == "chain" else None)))
        if bpv > 1:
            phi_edge |= (pairs // 2) % ppb == 0
            phi_inside |= (pairs // 2) % ppb != 0
            ragged |= pairs % ppb != 0
    assert seen >= {("A", 0), ("A", 1), ("B", None), ("tree2", None), ("tree4", None), ("tree8", None), ("chain", 1), ("chain", 2)}, seen
    assert phi_edge and phi_inside and ragged
    assert shim.plan(256, 4, 65) == (2560, 7) and shim.plan(64, 5, 1) == (256, 13)


@pytest.mark.parametrize("npoints,wbits,nvec", DIGIT_CASES)
def test_sums_from_random_digits(shim, src, npoints, wbits, nvec):
    a, table, kinds = shared_table(shim, src, npoints, wbits)
    want = [src.compressed(gx.digit_sum(d, a, npoints, wbits)) for d in kinds]
    assert want[1] == gx.INF48 and want[2] != gx.INF48
    order = period7(nvec)
    check_sums(from_digits(shim, table, npoints, wbits, kinds, order), want, order, "(%d, %d) x %d" % (npoints, wbits, nvec))


# ---- 3. sums from digits, solved bases ----

def disjoint_lanes(shape, block, lanes, count, used, need):
    """`count` lanes of `lanes` whose first `need` pairs of `block` read bases nobody else reads"""
    out = []
    for l in lanes:
        idx = [shape.pair(q)[0] for q in shape.lane_pairs(block, l)[:need]]
        if len(idx) == need and len(set(idx)) == need and not used & set(idx):
            used |= set(idx)
            out.append(l)
            if len(out) == count:
                return out
    pytest.fail("no %d lanes with disjoint bases" % count)


def event_vector(shape, rnd, waves):
    """a digit vector and the events wanted of it: in each of the given waves (lists of lanes) a doubling, a
    cancellation (the lane ends at infinity), a cancellation that an addition follows -- between them with both yneg
    states before the event -- and, where the block that holds the phi boundary has lanes on both sides, a doubling on
    the first addition after phi"""
    half = 1 << (shape.c - 1)
    d = [rnd.choice([v for v in range(-half, half + 1) if v]) for _ in range(shape.pairs)]
    per_lane = len(shape.lane_pairs(0, 0))
    wanted, used = [], set()
    plans = [[("double", True), ("cancel", False), ("cancel_go_on", True)], [("double", False), ("cancel", True), ("cancel_go_on", False)]]
    for lanes, plan in zip(waves, plans):
        plan = [(k, y) for k, y in plan if (1 if y else 2) + (2 if k == "cancel_go_on" else 1) <= per_lane]
        for (kind, yneg), l in zip(plan, disjoint_lanes(shape, 0, lanes, len(plan), used, min(per_lane, 4))):
            step = 1 if yneg else 2
            keep = step + (2 if kind == "cancel_go_on" else 1)
            for q in shape.lane_pairs(0, l)[keep:]:
                d[q] = 0
            wanted.append({"block": 0, "lane": l, "step": step, "kind": kind, "yneg": yneg})
    bphi = shape.phi_pairs // shape.ppb
    for lanes, before in zip(waves, (1, 2)):
        for l in lanes:
            pairs = shape.lane_pairs(bphi, l)
            lo = [q for q in pairs if q < shape.phi_pairs]
            hi = [q for q in pairs if q >= shape.phi_pairs]
            idx = {shape.pair(q)[0] for q in lo[-before:] + hi[:1]}
            if len(lo) >= before and hi and len(idx) == before + 1 and not used & idx and not (bphi == 0 and any(w["lane"] == l for w in wanted)):
                used |= idx
                for q in lo[:-before] + hi[1:]:
                    d[q] = 0
                wanted.append({"block": bphi, "lane": l, "step": 0, "kind": "after_phi", "yneg": before == 1})
                break
    return d, wanted


@pytest.mark.parametrize("nvec", [40, 57, 1024])
def test_solved_bases_force_doubling_and_cancellation_in_a_lane(shim, src, nvec):
    """(100, 4): a lane's base changes from pair to pair, so bases can be solved that make a chosen lane meet
    acc == entry and acc == -entry at a chosen addition.  nvec = 40: form A with three pairs a lane; 57: tree<8>, four
    pairs; 1024: the chain, one workgroup a vector, 25 pairs a lane -- every kind in the first and in the last wave,
    with both yneg states, an event on the first pair after phi, lanes that end at infinity"""
    n, c = 100, 4
    ppb, bpv = shim.plan(n, c, nvec)
    assert (ppb, bpv, run_form(ppb, bpv, nvec)) == {40: (768, 9, "A"), 57: (1024, 7, "tree8"), 1024: (6400, 1, "chain")}[nvec]
    shape = Shape(n, n, 256, ppb, c)
    rnd = random.Random(nvec)
    d, wanted = event_vector(shape, rnd, [list(range(1, 64)), list(range(192, 256))])
    a, seen = gx.solve_events(shape, d, wanted, [None] * n, rnd)
    kinds = {(w["kind"], w["lane"] < 64, w["yneg"]) for w in wanted}
    if nvec == 1024:   # everything the issue lists; the smaller shapes carry what their three or four pairs a lane allow
        for kind in gx.KINDS:
            assert {(kind, True), (kind, False)} <= {(k, first) for k, first, _ in kinds}, kind   # first and last wave
            assert {(kind, True), (kind, False)} <= {(k, y) for k, _, y in kinds}, kind           # both yneg states
    assert {"double", "cancel"} <= {w["kind"] for w in wanted}
    pred = gx.predict(shape, d, a)
    assert all((w["block"], w["lane"]) in pred["events"] for w in wanted)
    assert any(pred["lanes"][w["block"]][w["lane"]] == 0 for w in wanted if w["kind"] == "cancel")   # a lane that ends at infinity
    assert pred["total"] == gx.digit_sum(d, a, n, c)
    table = device_table(shim, src, a, c)
    vecs = [d] + digit_kinds(n, c, rnd)[:6]
    want = [src.compressed(gx.digit_sum(v, a, n, c)) for v in vecs]
    order = period7(nvec)
    check_sums(from_digits(shim, table, n, c, vecs, order), want, order, "events, nvec %d" % nvec)


# (nvec, form, the two blocks whose partial sums the fold adds first)
FOLD_CASES = [(1, "A", (0, 32)), (33, "B", (0, 8)), (513, "tree4", (0, 2)), (64, "tree8", (0, 4)), (4097, "chain", (0, 1))]


@pytest.mark.parametrize("nvec,form,partners", FOLD_CASES)
def test_solved_bases_make_lane_sums_and_block_partials_degenerate(shim, src, nvec, form, partners):
    """(256, 4): a lane keeps one base through all its windows, so bases are solved that make two block partial sums
    equal, opposite and infinite, a total infinite (c0 00...), and lane sums equal and opposite: lanes t and t + 128
    (what block_reduce_xyzz28_quad adds first), two lanes of a quad and two of a wave"""
    n, c = 256, 4
    ppb, bpv = shim.plan(n, c, nvec)
    assert run_form(ppb, bpv, nvec) == form and max(partners) < bpv
    shape = Shape(n, n, 256, ppb, c)
    rnd = random.Random(nvec + 7)
    half = 1 << (c - 1)
    dense = lambda: [rnd.choice([v for v in range(-half, half + 1) if v]) for _ in range(shape.pairs)]
    d_eq, d_op, d_inf, d_tot, d_lane = dense(), dense(), dense(), dense(), dense()
    x, y = partners
    cons = [lambda a: gx.block_sum(shape, d_eq, a, x) - gx.block_sum(shape, d_eq, a, y),
            lambda a: gx.block_sum(shape, d_op, a, x) + gx.block_sum(shape, d_op, a, y),
            lambda a: gx.block_sum(shape, d_inf, a, y),
            lambda a: gx.digit_sum(d_tot, a, n, c),
            lambda a: gx.lane_sum(shape, d_lane, a, 0, 5) - gx.lane_sum(shape, d_lane, a, 0, 133),
            lambda a: gx.lane_sum(shape, d_lane, a, 0, 6) + gx.lane_sum(shape, d_lane, a, 0, 134),
            lambda a: gx.lane_sum(shape, d_lane, a, 0, 12) - gx.lane_sum(shape, d_lane, a, 0, 13),
            lambda a: gx.lane_sum(shape, d_lane, a, 0, 16) + gx.lane_sum(shape, d_lane, a, 0, 48)]
    a = gx.solve_affine(cons, [rnd.randrange(1, R) for _ in range(n)], [20, 21, 22, 23, 133, 134, 13, 48])
    assert all(v for v in a)
    assert gx.block_sum(shape, d_eq, a, x) == gx.block_sum(shape, d_eq, a, y) != 0
    assert (gx.block_sum(shape, d_op, a, x) + gx.block_sum(shape, d_op, a, y)) % R == 0 != gx.block_sum(shape, d_op, a, x)
    assert gx.block_sum(shape, d_inf, a, y) == 0 != gx.block_sum(shape, d_inf, a, x)
    lanes = gx.predict(shape, d_lane, a)["lanes"][0]
    assert lanes[5] == lanes[133] != 0 and (lanes[6] + lanes[134]) % R == 0 and lanes[12] == lanes[13] and (lanes[16] + lanes[48]) % R == 0
    table = device_table(shim, src, a, c)
    vecs = [d_eq, d_op, d_inf, d_tot, d_lane, dense(), dense()]
    want = [src.compressed(gx.digit_sum(v, a, n, c)) for v in vecs]
    # (two opposite partial sums are the whole vector when there are only two: that total is infinity too)
    assert want[3] == gx.INF48 and [j for j, w in enumerate(want) if w == gx.INF48] == ([1, 3] if bpv == 2 else [3])
    order = period7(nvec)
    check_sums(from_digits(shim, table, n, c, vecs, order), want, order, "degenerate partials, form %s" % form)


# ---- 4. k_msm_small ----

SMALL_N, SMALL_C, SMALL_GROUPS = 192, 8, 3


def small_events(lpv, rnd):
    """the digit vector and the wanted events of one k_msm_small lane form, on group 1 (voff = 64)"""
    n, c = SMALL_N, SMALL_C
    half = 1 << (c - 1)
    shape = Shape(n, 64, lpv, 0, c, voff=64, lanes=lpv)
    d = [rnd.choice([v for v in range(-half, half + 1) if v]) for _ in range(shape.pairs)]
    wanted, used = [], set()
    plan = [("double", True), ("cancel", False), ("cancel_go_on", True), ("double", False), ("cancel", True), ("cancel_go_on", False)]
    for (kind, yneg), l in zip(plan, disjoint_lanes(shape, 0, range(lpv), len(plan), used, 4)):
        step = 1 if yneg else 2
        for q in shape.lane_pairs(0, l)[step + (2 if kind == "cancel_go_on" else 1):]:
            d[q] = 0
        wanted.append({"block": 0, "lane": l, "step": step, "kind": kind, "yneg": yneg})
    return shape, d, wanted


@pytest.mark.parametrize("nvec", [3, 4096, 4099, 8195, 65536])
def test_small_vector_sums(shim, src, nvec):
    """k_msm_small at ppv = 64 over a table of three groups (vecs_per_group = 3, so voff is 0, 64 and 128), with the
    default thresholds: one wave a vector below 8192 vectors (3, 4096, 4099), 16 lanes a vector with a partly filled
    last workgroup (8195), 8 lanes (65536).  In the 16- and 8-lane forms a lane walks four and eight bases: the events
    of the accumulate lanes are solved there.  In the one-wave form a lane keeps one base: lane sums equal and opposite
    (lanes l and l + 32, which the fold adds first), a total at infinity."""
    n, c, groups = SMALL_N, SMALL_C, SMALL_GROUPS
    rnd = random.Random(nvec)
    half = 1 << (c - 1)
    lpv = 64 if nvec < 8192 else (8 if nvec >= 65536 else 16)
    a = [rnd.randrange(1, R) for _ in range(64)] + [None] * 64 + [rnd.randrange(1, R) for _ in range(64)]
    special_group = 1
    if lpv == 64:
        shape = Shape(n, 64, 64, 0, c, voff=64, lanes=64)
        d = [rnd.choice([v for v in range(-half, half + 1) if v]) for _ in range(shape.pairs)]
        d_tot = [rnd.randint(-half, half) for _ in range(shape.pairs)]
        a[64:128] = [rnd.randrange(1, R) for _ in range(64)]
        a = gx.solve_affine([lambda a: gx.lane_sum(shape, d, a, 0, 3) - gx.lane_sum(shape, d, a, 0, 35),
                             lambda a: gx.lane_sum(shape, d, a, 0, 4) + gx.lane_sum(shape, d, a, 0, 36),
                             lambda a: gx.lane_sum(shape, d, a, 0, 8) - gx.lane_sum(shape, d, a, 0, 9),
                             lambda a: gx.digit_sum(d_tot, a, 64, c, voff=64)], a, [64 + 35, 64 + 36, 64 + 9, 64 + 50])
        lanes = gx.predict(shape, d, a)["lanes"][0]
        assert lanes[3] == lanes[35] != 0 and (lanes[4] + lanes[36]) % R == 0 and lanes[8] == lanes[9]
        special = [d, d_tot]
    else:
        shape, d, wanted = small_events(lpv, rnd)
        a, _ = gx.solve_events(shape, d, wanted, a, rnd)
        pred = gx.predict(shape, d, a)
        assert all((0, w["lane"]) in pred["events"] for w in wanted) and len(wanted) == 6
        assert any(pred["lanes"][0][w["lane"]] == 0 for w in wanted if w["kind"] == "cancel")
        special = [d]
    table = device_table(shim, src, a, c)
    pairs = 2 * gx.twin_for(c) * 64
    kinds = [[rnd.randint(-half, half) for _ in range(pairs)] for _ in range(5)] + [[0] * pairs, [rnd.choice((-half, half)) for _ in range(pairs)]]
    vecs = kinds + special
    # vector v takes kind (3 v) % 7, but the vectors of group 1 at the two ends and in the middle take the special ones
    order = period7(nvec)
    spots = sorted({v for v in (1, 4, nvec // 2 // 3 * 3 + 1, (nvec - 1) // 3 * 3 - 2, (nvec - 1) // 3 * 3 + 1) if 0 <= v < nvec and v % groups == special_group})
    assert spots
    for k, v in enumerate(spots):
        order[v] = 7 + k % len(special)
    packed = [pack(v) for v in vecs]
    out = guarded(192 * nvec, 192 * 2)
    assert shim.call("gs_msm_small", out, SZ(nvec + 2), table, SZ(len(table)), n, c, b"".join(packed[j] for j in order), SZ(nvec), 64, groups) == 0
    guard_intact(out, 192 * nvec, "small sums")
    want, raw = {}, out.raw
    for v, j in enumerate(order):
        key = (j, v % groups)
        if key not in want:
            want[key] = src.raw(gx.digit_sum(vecs[j], a, 64, c, voff=64 * (v % groups)))
        assert gx.xyzz_is(raw[192 * v:192 * v + 192], want[key]), "vector %d (kind %d, group %d)" % (v, j, v % groups)
    if lpv == 64 and nvec > 3:
        assert want[(8, 1)] == gx.ZERO_AFFINE   # the total at infinity
    # the first special vector once more as a point: x / zz, y / zzz
    assert gx.xyzz_point(raw[192 * spots[0]:192 * spots[0] + 192]) == gx.affine_point(want[(7, 1)])


# ---- 5. recoding, and the commitment calls over chosen bases ----

def edge_scalars(c, rnd):
    half, twin = 1 << (c - 1), gx.twin_for(c)
    vals = [0, 1, R - 1, R - 2, LAMBDA, LAMBDA + 1, LAMBDA - 1, LAMBDA // 2, LAMBDA // 2 + 1, R - LAMBDA,
            (LAMBDA + 1) * (LAMBDA // 2), (LAMBDA + 1) * (LAMBDA // 2 + 1) % R, LAMBDA * LAMBDA % R]
    # half-scalars whose windows are all exactly +-half (the recoding's carry rule), in both halves and signs
    m = sum(half << (c * w) for w in range(0, twin - 1, 2))
    m2 = sum((half - 1) << (c * w) for w in range(twin - 1))
    for x in (m, m2, m >> 1):
        for y in (m, m2, 1, 0):
            for sx in (1, -1):
                for sy in (1, -1):
                    vals.append((sx * x + LAMBDA * sy * y) % R)
    return vals + [rnd.randrange(R) for _ in range(16)]


def check_recoding(digits, scalars, nvec, n, c):
    """digits[vec][w][i]: every scalar's digits are at most 2^(c-1) in size and give (k1, k2) with k1 + lambda k2 = k"""
    nwin, half = 2 * gx.twin_for(c), 1 << (c - 1)
    assert len(digits) == nvec * nwin * n
    assert max(digits) <= half and min(digits) >= -half
    for v in range(nvec):
        for i in range(n):
            d = [digits[(v * nwin + w) * n + i] for w in range(nwin)]
            k1, k2 = gx.digits_value(d, c)
            assert (k1 + LAMBDA * k2 - scalars[v][i]) % R == 0, "vector %d, scalar %d: digits %r" % (v, i, d)


def commit_bases(src, rnd):
    """4096 bases (i + 1) k G by the oracle's additions, with infinity at the ends and in the middle and a repeat"""
    k = rnd.randrange(1, R)
    a = [(i + 1) * k % R for i in range(4096)]
    raw = bytearray(src.chain_raw(src.jac(k), 4096))
    for i in (0, 2048, 4095):
        a[i] = 0
        raw[96 * i:96 * i + 96] = bytes(96)
    a[17] = a[16]
    raw[96 * 17:96 * 18] = raw[96 * 16:96 * 17]
    return a, bytes(raw)


def test_commit_raw_recodes_and_sums(shim, src):
    """msm_commit_table_raw_device over 4096 chosen bases: the digits k_raw_digits left (the recoding property on the
    edge scalars of both halves and on random ones, the [vec][w][i] layout) and the commitments sum k_i a_i"""
    c, n = 4, 3
    rnd = random.Random(4844)
    a, raw = commit_bases(src, rnd)
    edge = edge_scalars(c, rnd)
    scalars = [[edge[(i + 5 * v) % len(edge)] if i % 3 == 0 else rnd.randrange(R) for i in range(4096)] for v in range(n)]
    scalars[1] = [0] * 4096
    out = guarded(48 * n, 96)
    nwin = 2 * gx.twin_for(c)
    digits = C.create_string_buffer(n * nwin * 4096 * 2)
    assert shim.call("gs_commit_raw", out, SZ(len(out)), digits, raw, c, gx.le_words([k for v in scalars for k in v]), SZ(n)) == 0
    guard_intact(out, 48 * n, "commitments")
    check_recoding(unpack(digits.raw), scalars, n, 4096, c)
    for v in range(n):
        assert out.raw[48 * v:48 * v + 48] == src.compressed(gx.scalar_sum(scalars[v], a)), v
    assert out.raw[48:96] == gx.INF48


def test_commit_blobs_flags_a_non_canonical_element_and_nothing_else(shim, src):
    """commit_blobs_enqueue: an element >= r (at element 0, at element 4095, on both sides of a blob edge) sets its
    blob's status only, gives all-zero digits there and leaves the neighbours' digits as the recoding makes them"""
    c, n = 4, 4
    rnd = random.Random(7594)
    a, raw = commit_bases(src, rnd)
    edge = edge_scalars(c, rnd)
    scalars = [[edge[(i + 7 * v) % len(edge)] if i % 5 == 0 else rnd.randrange(R) for i in range(4096)] for v in range(n)]
    sent = [list(v) for v in scalars]
    bad = {(1, 0): R, (1, 4095): 2 ** 256 - 1, (2, 0): R + 1}   # blob 1 | blob 2: both sides of their edge
    for (v, i), val in bad.items():
        sent[v][i] = val
        scalars[v][i] = 0   # what the digits must say there
    blobs = b"".join(k.to_bytes(32, "big") for v in sent for k in v)
    out, status = guarded(48 * n, 96), guarded(n, 1)
    nwin = 2 * gx.twin_for(c)
    digits = C.create_string_buffer(n * nwin * 4096 * 2)
    assert shim.call("gs_commit_blobs", out, SZ(len(out)), status, digits, raw, c, blobs, SZ(n)) == 0
    guard_intact(out, 48 * n, "commitments")
    assert status.raw == bytes([0, 1, 1, 0, GUARD])
    got = unpack(digits.raw)
    check_recoding(got, scalars, n, 4096, c)
    for (v, i) in bad:
        assert all(got[(v * nwin + w) * 4096 + i] == 0 for w in range(nwin))
    for v in (0, 3):
        assert out.raw[48 * v:48 * v + 48] == src.compressed(gx.scalar_sum(scalars[v], a)), v


# ---- 6. call-time table sums ----

CALL_POINTS = [1, 3, 24, 100, 256, 300]
CALL_C = 6


def call_event_scalars(n, ppb, a, k, rnd, used):
    """related bases and scalars that make a lane of k_msm_accumulate_x28 meet acc == entry and acc == -entry: the lane
    adds pair q2 and then q1 = q2 + 256; with a[i1] = A, a[i2] = 64^(w1 - w2) A and one digit d in window tw2 of k[i2]
    and in window tw1 of k[i1], both pairs select d 64^tw1 A.  Where the phi boundary lies inside a block the same
    across it: the k2-half sum goes through phi, so the base is lambda 64^(..) A."""
    twin = gx.twin_for(CALL_C)
    pairs, phi = 2 * twin * n, twin * n
    made = []
    for kind in ("double", "cancel", "phi_double"):
        for q2 in range(phi if kind != "phi_double" else max(0, phi - 256), pairs - 256 if kind != "phi_double" else phi):
            q1 = q2 + 256
            if q1 >= pairs or q2 // ppb != q1 // ppb:
                continue
            w2, i2, w1, i1 = q2 // n, q2 % n, q1 // n, q1 % n
            tw2, tw1 = w2 % twin, w1 % twin
            if i1 == i2 or {i1, i2} & used or a[i1] == 0 or a[i2] == 0 or tw1 > 18 or (kind != "phi_double" and tw2 > 18) or (kind == "phi_double" and q1 < phi):
                continue
            d = 1 if kind == "phi_double" else rnd.randint(1, 31)   # (k2 = d 64^tw2 has to stay a half-scalar)
            big = rnd.randrange(1, R)
            if kind == "phi_double":
                a[i2] = big
                a[i1] = LAMBDA * pow(64, tw2, R) * pow(pow(64, tw1, R), -1, R) * big % R
                k[i2] = LAMBDA * (d << (CALL_C * tw2)) % R
                k[i1] = d << (CALL_C * tw1)
            else:
                a[i1] = big
                a[i2] = pow(64, w1 - w2, R) * big % R
                k[i2] = d << (CALL_C * tw2)
                k[i1] = (d << (CALL_C * tw1)) if kind == "double" else R - (d << (CALL_C * tw1))
            used |= {i1, i2}
            made.append((kind, q2 // ppb, q2 % ppb % 256))
            break
    return made


@pytest.mark.parametrize("npoints", CALL_POINTS)
def test_call_time_table_sums(shim, src, npoints):
    """a 6-bit X28 table over caller points and sums of 1, 3 and 4 scalar vectors over it: infinity at the ends and in
    the middle, P and -P with equal scalars, related bases (P, 64^j P and P, lambda P) with scalars that make a lane
    meet acc == entry and acc == -entry, a vector of zero scalars, a total at infinity, every point the same; the digits
    k_raw_digits_n left are checked as a recoding"""
    n, c = npoints, CALL_C
    rnd = random.Random(npoints)
    ppb, bpv = shim.plan(n, c, 4, fixed=0)
    assert bpv == {1: 1, 3: 1, 24: 3, 100: 9, 256: 22, 300: 26}[n]
    phi = gx.twin_for(c) * n
    assert (phi % ppb == 0) == (n == 256) or bpv == 1
    a = special_bases(n, rnd)
    edge = edge_scalars(c, rnd)
    k_rand = [edge[i % len(edge)] if i % 2 else rnd.randrange(R) for i in range(n)]
    if n >= 16:
        k_rand[7] = k_rand[6]   # P and -P with equal scalars
    k_ev = [rnd.randrange(R) for _ in range(n)]
    made = call_event_scalars(n, ppb, a, k_ev, rnd, {0, n // 2, n - 1, 1, 3, 4, 5, 6, 7, 9}) if ppb >= 512 and n not in (256,) else []
    k_tot = [rnd.randrange(R) for _ in range(n)]
    free = next(i for i in range(n - 1, -1, -1) if a[i])
    k_tot[free] = -sum(x * y for i, (x, y) in enumerate(zip(k_tot, a)) if i != free) * pow(a[free], -1, R) % R
    vectors = [k_ev, [0] * n, k_tot, k_rand]
    pts = bases_raw(src, a)
    nwin = 2 * gx.twin_for(c)
    for nvec in (4, 3, 1):
        assert shim.plan(n, c, nvec, fixed=0) == (ppb, bpv)
        sums = guarded(192 * nvec, 192)
        digits = C.create_string_buffer(nvec * nwin * n * 2)
        assert shim.call("gs_table_sums", sums, SZ(nvec + 1), digits, pts, n, c, gx.le_words([x for v in vectors[:nvec] for x in v]), SZ(nvec), 1, None) == 0
        guard_intact(sums, 192 * nvec, "table sums")
        got = unpack(digits.raw)
        check_recoding(got, vectors, nvec, n, c)
        for v in range(nvec):
            want = src.point(gx.scalar_sum(vectors[v], a))
            assert gx.xyzz_point(sums.raw[192 * v:192 * v + 192]) == want, "vector %d of %d" % (v, nvec)
        if nvec >= 3:
            assert sums.raw[192:384] == gx.ZERO_XYZZ and sums.raw[384:576] == gx.ZERO_XYZZ   # zero scalars; a total at infinity
        if nvec == 4 and made:
            # the events really happen in the lane walk over the digits the device made
            shape = Shape(n, n, 256, ppb, c)
            for kind, block, lane in made:
                _, ev = gx.replay_lane(shape, list(got[:nwin * n]), a, block, lane)
                assert any(k == ("cancel" if kind == "cancel" else "double") and (phi_ or kind != "phi_double") for _, k, _, phi_ in ev), (kind, ev)
    if n in (24, 100, 300):
        assert {"double", "cancel"} <= {m[0] for m in made}
    if n == 300:
        assert "phi_double" in {m[0] for m in made}
    # every point the same
    same = [a[free]] * n
    sums = guarded(192, 192)
    digits = C.create_string_buffer(nwin * n * 2)
    assert shim.call("gs_table_sums", sums, SZ(2), digits, bases_raw(src, same), n, c, gx.le_words(k_rand), SZ(1), 1, None) == 0
    guard_intact(sums, 192, "table sums")
    assert gx.xyzz_point(sums.raw[:192]) == src.point(gx.scalar_sum(k_rand, same))


def test_call_time_sums_read_all_of_zz(shim, src):
    """An X28 entry is at infinity when ALL of zz is zero.  No honest build produces a zz whose low limbs alone are zero
    (a chance of 2^-224), so the table comes from the test here: one point, every entry (e + 1) 64^w a G with zz = 1, but
    the first entry in a representation whose zz has its eight low limbs zero and is not zero.  An entry that is all
    zero is still skipped."""
    c, a = CALL_C, 0x1234567
    twin, half = gx.twin_for(c), 1 << (c - 1)
    entries = []
    for w in range(twin):
        base = src.jac(a << (c * w))
        row = src.chain_raw(base, half)
        entries += [gx.x28_raw(gx.affine_point(row[96 * e:96 * e + 96])) for e in range(half)]
    t = 1
    while True:   # zz = z^2 whose 2^392-domain value is t 2^224
        zz = (t << 224) * pow(gx.M392, -1, gx.P) % gx.P
        z = gx.sqrt_fp(zz)
        if z is not None and (t << 224) < gx.P:
            break
        t += 1
    entries[0] = gx.x28_raw(src.point(a), z)
    assert entries[0][112:144] == bytes(32) and entries[0][144:168] != bytes(24)
    entries[2] = bytes(224)   # 3 a G declared at infinity
    scalars = [[1], [2], [1 + (2 << c)], [3], [3 + (1 << (2 * c))]]
    sums, digits = guarded(192 * 5, 192), C.create_string_buffer(5 * 2 * twin * 2)
    assert shim.call("gs_table_sums", sums, SZ(6), digits, bytes(96), 1, c, gx.le_words([k[0] for k in scalars]), SZ(5), 0, b"".join(entries)) == 0
    guard_intact(sums, 192 * 5, "table sums")
    check_recoding(unpack(digits.raw), scalars, 5, 1, c)
    for v, k in enumerate([1, 2, 1 + (2 << c), 0, 1 << (2 * c)]):
        assert gx.xyzz_point(sums.raw[192 * v:192 * v + 192]) == src.point(k * a), v


# ---- 7. batch_to_affine_device ----

_affine_pattern = {}


def affine_pattern(src):
    """301 points (odd: coprime to every run length): a stretch of 255 at infinity -- whatever the alignment, a whole
    run of 128 -- then finite points with z != 1 between single infinities"""
    if not _affine_pattern:
        rnd = random.Random(301)
        ks = [rnd.randrange(1, R) for _ in range(12)]
        tail = [ks[i % 12] if i % 5 != 3 else 0 for i in range(45)]
        dl = [ks[0]] + [0] * 255 + tail
        assert len(dl) == 301
        xyzz = [gx.xyzz_raw(src.point(k), rnd.randrange(2, gx.P)) for k in dl]
        _affine_pattern.update(xyzz=xyzz, aff=[src.raw(k) for k in dl])
    return _affine_pattern["xyzz"], _affine_pattern["aff"]


@pytest.mark.parametrize("n", [1, 4096, 4097, 4100, 16384, 1 << 20])
def test_batch_to_affine(shim, src, n):
    """run lengths 1 (n <= 4096), 4, 16 and 128; non-unit zz, infinity single, first and last in a run, whole runs at
    infinity; the guard past the end intact"""
    xyzz, aff = affine_pattern(src)
    reps = n // 301 + 1
    data = (b"".join(xyzz) * reps)[:192 * n]
    want = (b"".join(aff) * reps)[:96 * n]
    out = guarded(96 * n, 96 * 130)
    assert shim.call("gs_batch_to_affine", out, SZ(n + 130), data, SZ(n)) == 0
    guard_intact(out, 96 * n, "affine points")
    got = out.raw[:96 * n]
    if got != want:
        at = next(i for i in range(n) if got[96 * i:96 * i + 96] != want[96 * i:96 * i + 96])
        pytest.fail("point %d of %d is %s, expected %s" % (at, n, got[96 * at:96 * at + 96].hex(), want[96 * at:96 * at + 96].hex()))


# ---- 8. ladders and buckets, several jobs ----

def make_jobs(sizes, rnd, pool):
    """per job (dlogs, scalars): duplicates and P, -P in every job of two or more terms; job kinds by position"""
    jobs = []
    for j, size in enumerate(sizes):
        a = [pool[rnd.randrange(len(pool))] for _ in range(size)]
        k = [rnd.randrange(R) for _ in range(size)]
        if size >= 4:
            a[1], k[1] = a[0], k[0]          # the same term twice
            a[3] = R - a[2]                  # P, -P
        jobs.append((a, k))
    return jobs


JOB_LAYOUTS = [[200], [65, 0, 64], [63, 1, 64, 200], [1, 200, 65]]


@pytest.mark.parametrize("layout", range(len(JOB_LAYOUTS)))
def test_ladders_and_buckets_over_several_jobs(shim, src, layout):
    """lincomb_multi_device (32 terms a partial and the quad form, 8 terms) and bucket_msm_enqueue (5- and 8-bit
    buckets) over 1, 3 and 4 jobs of 0, 1, 63, 64, 65 and 200 terms: a job all at infinity, a job of zero scalars, a
    job whose sum is infinity next to one whose sum is not, duplicates, P and -P"""
    sizes = JOB_LAYOUTS[layout]
    rnd = random.Random(layout + 50)
    pool = [rnd.randrange(1, R) for _ in range(24)]
    jobs = make_jobs(sizes, rnd, pool)
    big = [j for j, s in enumerate(sizes) if s >= 63]
    if len(big) >= 2:   # a sum at infinity next to one that is not
        a, k = jobs[big[0]]
        k[-1] = -sum(x * y for x, y in zip(a[:-1], k[:-1])) * pow(a[-1], -1, R) % R
    if len(big) >= 3:
        jobs[big[1]] = ([0] * sizes[big[1]], jobs[big[1]][1])                 # all at infinity
        jobs[big[2]] = (jobs[big[2]][0], [0] * sizes[big[2]])                 # zero scalars
    want = b"".join(src.raw(gx.scalar_sum(k, a)) for a, k in jobs)
    njobs = len(jobs)
    if len(big) >= 2:
        assert want[96 * big[0]:96 * big[0] + 96] == gx.ZERO_AFFINE
    # ladders: every job padded to a multiple of 64 with infinity and zero scalars
    pts, sc, padded = b"", b"", []
    for a, k in jobs:
        pad = -len(a) % 64
        pts += bases_raw(src, a + [0] * pad)
        sc += gx.le_words(k + [0] * pad)
        padded.append(len(a) + pad)
    total = sum(padded)
    for quad in (0, 1):
        per = 8 if quad else 32
        off = [0]
        for p in padded:
            off.append(off[-1] + p // per)
        out = guarded(96 * njobs, 96)
        assert shim.call("gs_lincomb_multi", out, pts, sc, SZ(total), (C.c_uint32 * len(off))(*off), njobs, quad) == 0
        guard_intact(out, 96 * njobs, "lincomb")
        assert out.raw[:96 * njobs] == want, "quad %d" % quad
    # buckets: the jobs back to back
    pts = b"".join(bases_raw(src, a) for a, _ in jobs)
    sc = b"".join(gx.le_words(k) for _, k in jobs)
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    for wbits in (5, 8):
        out = guarded(96 * njobs, 96)
        assert shim.call("gs_bucket_msm", out, pts, sc, SZ(off[-1]), (C.c_uint32 * len(off))(*off), njobs, wbits) == 0
        guard_intact(out, 96 * njobs, "buckets")
        assert out.raw[:96 * njobs] == want, "wbits %d" % wbits


def test_bucket_lane_overflows_its_match_list(shim, src):
    """more than six equal digits in one bucket lane: a job of 520 terms whose terms 3, 67, 131, ... (one lane of the
    sweep) carry the same scalar, so the lane records six matches and adds the rest on the spot; between two other
    jobs"""
    rnd = random.Random(99)
    pool = [rnd.randrange(1, R) for _ in range(16)]
    jobs = make_jobs([65, 520, 64], rnd, pool)
    a, k = jobs[1]
    for i in range(3, 520, 64):
        k[i] = 5 + (9 << 8) + LAMBDA * 3 % R
        a[i] = pool[i // 64 % len(pool)] if i > 67 else a[3]   # (two of them the same point: a doubling in the bucket)
    want = b"".join(src.raw(gx.scalar_sum(k_, a_)) for a_, k_ in jobs)
    pts = b"".join(bases_raw(src, a_) for a_, _ in jobs)
    sc = b"".join(gx.le_words(k_) for _, k_ in jobs)
    off = [0, 65, 585, 649]
    for wbits in (5, 8):
        out = guarded(96 * 3, 96)
        assert shim.call("gs_bucket_msm", out, pts, sc, SZ(649), (C.c_uint32 * 4)(*off), 3, wbits) == 0
        guard_intact(out, 96 * 3, "buckets")
        assert out.raw[:96 * 3] == want, "wbits %d" % wbits


# ---- 9. the segmented scan ----

@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_segmented_prefix_scan(shim, src, n):
    """nseg = 2 and 3 arrays of n points with different data each: every prefix against the segment's own running integer
    sum.  The summands repeat with a short period and add up to zero over it, so the running sums take a few values
    (one scalar multiplication each); infinity and P, -P lie across the tile edges (the periods are odd)."""
    rnd = random.Random(n)
    for nseg in (2, 3):
        data, want = [], []
        for s in range(nseg):
            k1, k2 = rnd.randrange(1, R), rnd.randrange(1, R)
            period = [[k1, R - k1, 0, k2, k1, R - k1 - k2, 0], [k2, k2, 0, 0, R - k2, k1, R - k1 - k2, k2, R - k2],
                      [0, k1, k1, R - 2 * k1 % R, k2, R - k2, 0, 0, k1, k2, R - k1 - k2]][s]
            assert sum(period) % R == 0 and len(period) % 2 == 1
            raws = [gx.xyzz_raw(src.point(k), rnd.randrange(2, gx.P)) for k in period]
            run, pref = 0, []
            for k in period:
                run = (run + k) % R
                pref.append(src.raw(run))
            reps = n // len(period) + 1
            data.append((b"".join(raws) * reps)[:192 * n])
            want += (pref * reps)[:n]
        buf = C.create_string_buffer(b"".join(data) + bytes([GUARD]) * 192 * 2, 192 * (nseg * n + 2))
        assert shim.call("gs_prefix_scan", buf, SZ(nseg * n + 2), SZ(n), SZ(nseg)) == 0
        guard_intact(buf, 192 * nseg * n, "scan")
        raw = buf.raw
        for i, w in enumerate(want):
            assert gx.xyzz_is(raw[192 * i:192 * i + 192], w), "segment %d of %d, prefix %d of %d" % (i // n, nseg, i % n, n)
        assert gx.xyzz_point(raw[192 * (n - 1):192 * n]) == gx.affine_point(want[n - 1])


# ---- 10. refusals ----

def test_refusals(shim, src):
    """a window width outside what build_fixed_base_table (2 .. 16) and bucket_msm_enqueue (4 .. 16) state, sums over a
    table that was never built, and no vectors: each refuses the call, and the output comes back as it went up"""
    a = [5, 7]
    raw = bases_raw(src, a)
    for wbits in (1, 17):
        buf = guarded(96 * 64, 96)
        assert shim.call("gs_build_table", buf, SZ(len(buf)), raw, 2, wbits) == 1
        guard_intact(buf, 0, "refused table")
    sc = gx.le_words([3, 4])
    for wbits in (3, 17):
        out = guarded(96, 96)
        assert shim.call("gs_bucket_msm", out, raw, sc, SZ(2), (C.c_uint32 * 2)(0, 2), 1, wbits) == 2
        guard_intact(out, 0, "refused buckets")
    sums, digits = guarded(192, 192), C.create_string_buffer(2 * gx.twin_for(6) * 2 * 2)
    assert shim.call("gs_table_sums", sums, SZ(2), digits, raw, 2, 6, sc, SZ(1), 0, None) == 2      # no table
    guard_intact(sums, 0, "refused sums")
    assert shim.call("gs_table_sums", sums, SZ(2), digits, raw, 2, 6, sc, SZ(0), 1, None) == 2      # nvec = 0
    guard_intact(sums, 0, "refused sums")
    table = device_table(shim, src, a, 4)
    out = guarded(48, 48)
    d = pack([1] * (2 * gx.twin_for(4) * 2))
    assert shim.call("gs_msm_from_digits", out, SZ(len(out)), table, SZ(0), 2, 4, d, SZ(1)) == 2          # no table
    guard_intact(out, 0, "refused sum")
    assert shim.call("gs_msm_from_digits", out, SZ(len(out)), table, SZ(len(table)), 2, 4, d, SZ(0)) == 0   # nvec = 0: nothing to do
    guard_intact(out, 0, "empty sum")
    assert shim.call("gs_msm_from_digits", out, SZ(len(out)), table, SZ(len(table)), 2, 4, d, SZ(1)) == 0
    assert out.raw[:48] == src.compressed(gx.digit_sum([1] * (2 * gx.twin_for(4) * 2), a, 2, 4))
