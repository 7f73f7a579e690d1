"""What can be said about tests/test_gpu_g1_stages.py without a GPU.

The references of tests/g1_expect.py, each by a second route: the oracle's points against the Python curve model of
tests/g1_points.py, the digit-vector formula against the host replay of the accumulate kernels (hs_msm_glv_emulate over
digits from hs_recode_signed_128) and the oracle's naive linear combination, the table-entry encoding against the host
shim's field product, a table against plain multiples, and the solvers by replaying a lane step by step with the
oracle's additions: an event is a step whose accumulator really has the entry's x.

The shim (tests/native/g1_shim.hip), as tests/test_poly_expect_cpu.py checks its shim: libg1_shim.so cross-compiles
for gfx950 and exports every gs_* function the GPU module binds, it is linked from the product's own object files, and
none of it appears in libckzg_hip.so, whose export list is still exactly exports.map."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import g1_expect as gx
import g1_points as gp
from g1_expect import R, LAMBDA, Shape
from conftest import ROOT, SHIM_SO, ORACLE_SO
from test_gpu_g1_stages import G1_FUNCTIONS, G1_SHIM_SO, edge_scalars, event_vector, small_events, call_event_scalars, special_bases
from test_abi_exports import declared_symbols
from test_stage_shim_cpu import _defined, test_the_test_aid_stays_out_of_the_product as _product_exports_are_the_map

PKG = os.path.join(ROOT, "c-kzg-4844_amd")


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "csrc/libhost_shim.so"])
    return C.CDLL(SHIM_SO)


@pytest.fixture(scope="module")
def src():
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    return gx.G1Source(C.CDLL(ORACLE_SO))


def host_digits(host, k, c):
    """the nwin digits of one scalar by the product's own split and recoding, on the host"""
    twin = gx.twin_for(c)
    m1, m2, n1, n2 = (C.c_uint32 * 4)(), (C.c_uint32 * 4)(), C.c_int(), C.c_int()
    host.hs_glv_split_signed((C.c_uint32 * 8).from_buffer_copy(k.to_bytes(32, "little")), m1, C.byref(n1), m2, C.byref(n2))
    d1, d2 = (C.c_int16 * twin)(), (C.c_int16 * twin)()
    host.hs_recode_signed_128(d2, m2, n2.value, c, twin)
    host.hs_recode_signed_128(d1, m1, n1.value, c, twin)
    return list(d2) + list(d1)


# ---- the references ----

def test_the_oracle_points_are_the_python_model(src):
    rnd = random.Random(1)
    assert src.point(0) is gp.INF and src.raw(R) == gx.ZERO_AFFINE and src.point(1) == gp.G
    for k in (2, R - 1, LAMBDA, rnd.randrange(R)):
        pt = gp.mul(gp.G, k)
        assert src.point(k) == pt and src.raw(k) == gx.affine_raw(pt) and src.compressed(k) == gp.compress(pt)
    # phi is multiplication by LAMBDA: (beta x, y) with beta^3 = 1
    x, y = src.point(7)
    lx, ly = src.point(7 * LAMBDA)
    assert ly == y and lx != x and pow(lx * pow(x, -1, gp.P), 3, gp.P) == 1


def test_xyzz_forms(src):
    rnd = random.Random(2)
    pt = src.point(11)
    for z in (1, 2, rnd.randrange(2, gp.P)):
        b = gx.xyzz_raw(pt, z)
        assert gx.xyzz_point(b) == pt and gx.xyzz_is(b, src.raw(11)) and not gx.xyzz_is(b, src.raw(12))
    assert gx.xyzz_point(gx.ZERO_XYZZ) is gp.INF and gx.xyzz_is(gx.ZERO_XYZZ, gx.ZERO_AFFINE)
    assert not gx.xyzz_is(gx.xyzz_raw(pt, 3), gx.ZERO_AFFINE) and not gx.xyzz_is(gx.ZERO_XYZZ, src.raw(11))
    bad = bytearray(gx.xyzz_raw(pt, 5))
    bad[150] ^= 1   # zzz no longer the cube root's partner of zz
    assert not gx.xyzz_is(bytes(bad), src.raw(11))
    with pytest.raises(AssertionError):
        gx.xyzz_point(bytes(bad))
    # an X28 entry: fourteen limbs of 28 bits a coordinate, 2^392 domain
    e = gx.x28_raw(pt, 9)
    vals = [sum(int.from_bytes(e[56 * k + 4 * j:56 * k + 4 * j + 4], "little") << (28 * j) for j in range(14)) for k in range(4)]
    assert all(int.from_bytes(e[4 * j:4 * j + 4], "little") < 1 << 28 for j in range(56))
    assert vals == [v * gx.M392 % gp.P for v in (pt[0] * 81, pt[1] * 729, 81, 729)] and gx.x28_raw(gp.INF) == bytes(224)


def test_table_entry_encoding_is_the_host_field_product(host, src):
    """a table coordinate is the 2^384-domain coordinate times FP_MONT_2POW8, fully reduced"""
    with open(os.path.join(PKG, "csrc", "bls_consts32.h")) as f:
        words = re.search(r"FP_MONT_2POW8\[12\] = \{([^}]*)\}", f.read()).group(1)
    k8 = sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(words.split(",")))
    assert k8 == pow(2, 392, gp.P)
    host.hs_fp_mul.restype = None
    for k in (1, 5, R - 1):
        pt = src.point(k)
        want = gx.table_entry_raw(pt)
        for j in range(2):
            out = C.create_string_buffer(48)
            host.hs_fp_mul(out, gx.fp_raw(pt[j]), k8.to_bytes(48, "little"))
            assert out.raw == want[48 * j:48 * j + 48]
    assert gx.table_entry_raw(gp.INF) == bytes(96)


def test_table_is_plain_multiples(src):
    a, c = [3, 0, R - 1], 4
    tb = gx.table_raw(src, a, c)
    half, twin = 8, gx.twin_for(c)
    assert len(tb) == twin * 3 * half * 96
    for tw, i, e in ((0, 0, 0), (0, 0, 7), (1, 2, 3), (31, 0, 7), (31, 2, 0), (5, 1, 4)):
        at = ((tw * 3 + i) * half + e) * 96
        assert tb[at:at + 96] == gx.table_entry_raw(gp.mul(gp.G, (e + 1) * (a[i] << (c * tw)) % R)), (tw, i, e)


def test_digit_sum_is_the_host_replay_and_the_naive_sum(host, src):
    """hs_msm_glv_emulate runs msm_sum_pairs' walk with the product's own inline functions over the product's recoding;
    the digit-vector formula over the same digits, the scalar-vector formula and okzg_g1_lincomb_naive agree with it"""
    rnd = random.Random(3)
    lib = src.lib
    lib.okzg_g1_lincomb_naive.restype = None
    for c, n, lanes in ((4, 5, 3), (6, 7, 256), (5, 3, 1)):
        a = [rnd.randrange(1, R) for _ in range(n)]
        k = edge_scalars(c, rnd)[:n - 1] + [rnd.randrange(R)]
        rnd.shuffle(k)
        nwin = 2 * gx.twin_for(c)
        d = [0] * (nwin * n)
        for i, ki in enumerate(k):
            di = host_digits(host, ki, c)
            assert (gx.digits_value(di, c)[0] + LAMBDA * gx.digits_value(di, c)[1] - ki) % R == 0
            for w in range(nwin):
                d[w * n + i] = di[w]
        total = gx.digit_sum(d, a, n, c)
        assert total == gx.scalar_sum(k, a)
        out = C.create_string_buffer(144)
        host.hs_msm_glv_emulate(out, b"".join(src.raw(v) for v in a), gx.le_words(k), n, c, lanes)
        assert out.raw[:96] == src.raw(total)
        # the lane walk on discrete logarithms gives the same total
        shape = Shape(n, n, lanes, 0, c)
        assert gx.predict(shape, d, a)["total"] == total
        assert sum(gx.lane_sum(shape, d, a, 0, l) for l in range(lanes)) % R == total
        jacs = b"".join(src.jac(v).raw for v in a)
        frs = C.create_string_buffer(32 * n)
        for i, ki in enumerate(k):
            lib.ofr_from_raw(C.byref(frs, 32 * i), ki.to_bytes(32, "little"))
        res, aff = C.create_string_buffer(144), C.create_string_buffer(96)
        lib.okzg_g1_lincomb_naive(res, jacs, frs, C.c_size_t(n))
        lib.og1_to_affine(aff, res)
        assert aff.raw == src.raw(total)


def test_recoding_property_on_the_edge_scalars(host):
    for c in (4, 6, 8):
        for k in edge_scalars(c, random.Random(c)):
            d = host_digits(host, k, c)
            k1, k2 = gx.digits_value(d, c)
            assert (k1 + LAMBDA * k2 - k) % R == 0 and max(abs(v) for v in d) <= 1 << (c - 1)


# ---- the solvers ----

def walk_with_the_oracle(src, shape, d, a, block, lane):
    """the lane's additions with the oracle's points: [(kind, yneg before, after phi)] decided by COORDINATES -- the
    accumulator's affine x against the entry's -- and the lane's sum as an affine string"""
    lib = src.lib
    lam = C.create_string_buffer(32)
    lib.ofr_from_raw(lam, LAMBDA.to_bytes(32, "little"))
    acc, inf, yneg, out = C.create_string_buffer(144), True, False, []
    pairs = shape.lane_pairs(block, lane)
    phi_pending, just_phi = len(pairs) > 0 and pairs[0] < shape.phi_pairs, False
    aff = lambda j: (lambda b: (lib.og1_to_affine(b, j), b.raw)[1])(C.create_string_buffer(96))
    for q in pairs:
        if phi_pending and q >= shape.phi_pairs:
            if not inf:
                lib.og1_mul(acc, acc, lam)
                just_phi = True
            phi_pending = False
        if d[q] == 0:
            continue
        i, coef = shape.pair(q)
        entry = src.jac(d[q] * coef * a[i])
        e_aff = aff(entry)
        if e_aff == gx.ZERO_AFFINE:
            continue
        if inf:
            kind = "load"
        else:
            a_aff = aff(acc)
            kind = "add" if a_aff[:48] != e_aff[:48] else ("double" if a_aff[48:] == e_aff[48:] else "cancel")
        out.append((kind, yneg, just_phi))
        lib.og1_add(acc, acc, entry)
        inf = aff(acc) == gx.ZERO_AFFINE
        yneg = True if kind == "load" else (False if kind in ("double", "cancel") else not yneg)
        just_phi = False
    if phi_pending and not inf:
        lib.og1_mul(acc, acc, lam)
    return out, aff(acc)


def test_solved_events_are_real_coincidences_of_x(src):
    """the (100, 4) case of the GPU module that carries every kind: each wanted lane, walked with the oracle's
    additions, meets its event where the solver says, and ends where the solver predicts"""
    n, c, ppb = 100, 4, 6400
    shape = Shape(n, n, 256, ppb, c)
    rnd = random.Random(1024)
    d, wanted = event_vector(shape, rnd, [list(range(1, 64)), list(range(192, 256))])
    a, seen = gx.solve_events(shape, d, wanted, [None] * n, rnd)
    assert len(wanted) == 8
    for w in wanted:
        got, end = walk_with_the_oracle(src, shape, d, a, w["block"], w["lane"])
        dlog, ev = gx.replay_lane(shape, d, a, w["block"], w["lane"])
        assert [(k, y, p) for _, k, y, p in ev] == got and ev == seen[(w["block"], w["lane"])]
        assert end == src.raw(dlog)
        kind = "cancel" if w["kind"].startswith("cancel") else "double"
        if w["kind"] == "after_phi":
            assert (kind, w["yneg"], True) in got
        else:
            assert got[w["step"]] == (kind, w["yneg"], False)
        if w["kind"] == "cancel":
            assert end == gx.ZERO_AFFINE
        if w["kind"] == "cancel_go_on":
            assert len(got) > w["step"] + 1 and end != gx.ZERO_AFFINE
    # an unwanted lane has no event
    assert not [k for k, _, _ in walk_with_the_oracle(src, shape, d, a, 0, 100)[0] if k in ("double", "cancel")]


def test_small_form_events_are_real(src):
    for lpv in (16, 8):
        rnd = random.Random(lpv)
        shape, d, wanted = small_events(lpv, rnd)
        a, _ = gx.solve_events(shape, d, wanted, [rnd.randrange(1, R) for _ in range(64)] + [None] * 128, rnd)
        for w in wanted:
            got, end = walk_with_the_oracle(src, shape, d, a, 0, w["lane"])
            assert got[w["step"]] == ("cancel" if w["kind"].startswith("cancel") else "double", w["yneg"], False)
            assert end == src.raw(gx.replay_lane(shape, d, a, 0, w["lane"])[0])


def test_call_time_event_scalars_recode_into_the_events(host):
    """the related bases and scalars of the call-time cases: over the product's own recoding (on the host) the lane walk
    meets acc == entry, acc == -entry and, across phi, acc == entry again"""
    c = 6
    for n, ppb in ((24, 512), (100, 512), (300, 512)):
        rnd = random.Random(n)
        a = special_bases(n, rnd)
        k = [rnd.randrange(R) for _ in range(n)]
        made = call_event_scalars(n, ppb, a, k, rnd, {0, n // 2, n - 1, 1, 3, 4, 5, 6, 7, 9})
        assert {m[0] for m in made} == {"double", "cancel", "phi_double"}
        nwin = 2 * gx.twin_for(c)
        d = [0] * (nwin * n)
        for i, ki in enumerate(k):
            for w, v in enumerate(host_digits(host, ki, c)):
                d[w * n + i] = v
        shape = Shape(n, n, 256, ppb, c)
        for kind, block, lane in made:
            _, ev = gx.replay_lane(shape, d, a, block, lane)
            assert any(k_ == ("cancel" if kind == "cancel" else "double") and (p or kind != "phi_double") for _, k_, _, p in ev)


def test_the_solvers_refuse_what_they_cannot_meet():
    shape = Shape(256, 256, 256, 1024, 4)   # a lane keeps one base: no base can make its accumulator meet an entry
    rnd = random.Random(5)
    d = [rnd.choice((-3, 2, 5)) for _ in range(shape.pairs)]
    with pytest.raises(gx.Refused):
        gx.solve_events(shape, d, [{"block": 0, "lane": 4, "step": 1, "kind": "double"}], [None] * 256, rnd)
    shape = Shape(100, 100, 256, 768, 4)
    d = [rnd.choice((-3, 2, 5)) for _ in range(shape.pairs)]
    for ev in ({"block": 0, "lane": 4, "step": 3, "kind": "double"},                      # three pairs a lane
               {"block": 0, "lane": 4, "step": 0, "kind": "cancel"},                      # nothing to cancel yet
               {"block": 0, "lane": 4, "step": 1, "kind": "double", "yneg": False},       # yneg is true after the load
               {"block": 0, "lane": 4, "step": 2, "kind": "cancel_go_on"},                # the lane's last pair
               {"block": 0, "lane": 200, "step": 0, "kind": "after_phi"},                 # the lane never crosses
               {"block": 0, "lane": 4, "step": 1, "kind": "triple"}):
        with pytest.raises(gx.Refused):
            gx.solve_events(shape, d, [ev], [None] * 100, rnd)
    with pytest.raises(gx.Refused):   # the base of the event is given
        gx.solve_events(shape, d, [{"block": 0, "lane": 4, "step": 1, "kind": "double"}], [7] * 100, rnd)
    a = [rnd.randrange(1, R) for _ in range(100)]
    with pytest.raises(gx.Refused):   # a constraint that does not hold a free base
        gx.solve_affine([lambda a_: gx.lane_sum(shape, d, a_, 0, 4) - 1], a, [99])
    with pytest.raises(gx.Refused):
        gx.solve_affine([lambda a_: a_[0]], a, [0, 1])
    got = gx.solve_affine([lambda a_: gx.lane_sum(shape, d, a_, 0, 4) - gx.lane_sum(shape, d, a_, 0, 5)], a, [4])
    assert gx.lane_sum(shape, d, got, 0, 4) == gx.lane_sum(shape, d, got, 0, 5) and got[5] == a[5]


# ---- the shim ----

@pytest.fixture(scope="module")
def g1_shim_path():
    if not os.path.exists(G1_SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "-j", "8", "libg1_shim.so"])
    return G1_SHIM_SO


def test_g1_shim_builds_and_exports_what_the_gpu_module_binds(g1_shim_path):
    names = _defined(g1_shim_path)
    for fn in G1_FUNCTIONS:
        assert fn in names, fn
    assert sorted(s for s in names if s.startswith("gs_")) == sorted(G1_FUNCTIONS)
    # linked with the product's objects, without its version script: the stage functions it calls are the product's
    assert "blob_to_kzg_commitment" in names
    for stage in ("build_fixed_base_table", "msm_from_digits_device", "msm_small_vectors_device", "table_sums_enqueue",
                  "batch_to_affine_device", "lincomb_multi_device", "bucket_msm_enqueue", "g1_prefix_scan_enqueue",
                  "msm_pairs_per_block"):
        assert any(stage in s for s in names), stage


def test_make_all_builds_the_g1_shim():
    with open(os.path.join(PKG, "Makefile")) as f:
        text = f.read()
    all_line = next(line for line in text.splitlines() if line.startswith("all:"))
    assert "libg1_shim.so" in all_line.split()
    rule = next(line for line in text.splitlines() if line.startswith("libg1_shim.so:"))
    assert "$(OBJS)" in rule
    link = text.split("\nlibg1_shim.so:")[1].splitlines()[1]
    assert "-Wl,-Bsymbolic" in link and "version-script" not in link
    clean = text.split("\nclean:")[1]
    assert "libg1_shim.so" in clean and "csrc/g1_shim.d" in text.split("-include")[-1]


def test_the_g1_shim_stays_out_of_the_product():
    _product_exports_are_the_map()   # the export list is exactly exports.map
    prod = _defined(os.path.join(PKG, "libckzg_hip.so"))
    assert not [s for s in prod if s.startswith("gs_")]
    assert not [n for n in declared_symbols() if n not in prod]   # (tests/test_abi_exports.py: every declared symbol)
