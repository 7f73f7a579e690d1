"""What can be said about tests/test_gpu_poly_stages.py without a GPU.

The references of tests/poly_expect.py, each by a second route: the opening quotient by interpolation and synthetic
division (which checks the transform reference on the way), evaluation against the Horner value of the coefficients,
the set factors against the host replay of coset_recover_factors.hpp, and evaluation against the host replays of the
two evaluation kernels on items of the GPU module.

The shim (tests/native/poly_shim.hip), as tests/test_stage_shim_cpu.py checks its shim: libpoly_shim.so cross-compiles
for gfx950 and exports every ps_* function the GPU module binds, it is linked from the product's own object files, and
none of it appears in libckzg_hip.so, whose export list is still exactly exports.map."""
import ctypes as C
import os
import random
import subprocess

import pytest

import poly_expect as px
import rlc_expect as rx
from rlc_expect import R
from conftest import ROOT, SHIM_SO
from test_gpu_poly_stages import POLY_FUNCTIONS, POLY_SHIM_SO, eval_items, quotient_items, recover_sets
from test_abi_exports import declared_symbols
from test_stage_shim_cpu import _defined, test_the_test_aid_stays_out_of_the_product as _product_exports_are_the_map

PKG = os.path.join(ROOT, "c-kzg-4844_amd")
R256 = pow(2, 256, R)


@pytest.fixture(scope="module")
def roots():
    return rx.roots_of_unity()


@pytest.fixture(scope="module")
def dom(roots):
    d = px.blob_domain(roots)
    return d, {w: i for i, w in enumerate(d)}


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "csrc/libhost_shim.so"])
    return C.CDLL(SHIM_SO)


# ---- the references ----

def test_dft_is_the_defining_sum(roots):
    rnd = random.Random(1)
    for logn in (0, 1, 2, 5):
        n = 1 << logn
        x = [rnd.randrange(R) for _ in range(n)]
        for inverse in (False, True):
            om = px.ntt_omega(roots, logn, inverse)
            assert om == pow(roots[1], (-1 if inverse else 1) * (8192 >> logn), R)
            assert px.dft(x, om) == [sum(x[i] * pow(om, i * k, R) for i in range(n)) % R for k in range(n)]
            want = [sum(x[i] * pow(om, i * k, R) for i in range(n)) % R for k in range(n)]
            dif = px.ntt(x, roots, logn, True, inverse, False)
            assert [dif[px.brp(k, logn)] for k in range(n)] == want
            dit = px.ntt([x[px.brp(i, logn)] for i in range(n)], roots, logn, False, inverse, False)
            assert dit == want
            assert px.ntt(x, roots, logn, True, inverse, True) == [v * pow(n, -1, R) % R for v in dif]


def test_dit_inverts_dif(roots):
    rnd = random.Random(2)
    for logn in (3, 7, 13):
        x = [rnd.randrange(R) for _ in range(1 << logn)]
        assert px.ntt(px.ntt(x, roots, logn, True, False, False), roots, logn, False, True, True) == x


def _quotient_by_division(poly, z, roots):
    """coefficients by the inverse transform, synthetic division by (x - z), the quotient's values by the forward one"""
    nat = [0] * 4096
    for i, v in enumerate(poly):
        nat[px.brp(i, 12)] = v
    coeffs = px.times_inv_n(px.dft(nat, roots[8192 - 2]), 12)
    quo, carry = [0] * 4096, 0
    for k in range(4095, -1, -1):
        quo[k], carry = carry, (coeffs[k] + carry * z) % R    # carry ends as the remainder p(z)
    vals = px.dft(quo, roots[2])
    return carry, [vals[px.brp(i, 12)] for i in range(4096)], coeffs


def test_quotient_and_evaluation_by_interpolation_and_division(roots, dom):
    d, index = dom
    polys, zs = quotient_items(d)
    for item in (0, 3, 7, 2, 11):   # z = 0; z = w_2 and w_4095 with p_i = y off m; all R - 1 at w_1; random
        y, m, q = px.quotient(polys[item], zs[item], d, index)
        y2, q2, coeffs = _quotient_by_division(polys[item], zs[item], roots)
        assert m == index.get(zs[item], -1)
        assert y == y2 == px.horner(coeffs, zs[item]), item
        assert q == q2, item


def test_gpu_module_polynomial_items_by_the_barycentric_formula(dom):
    """the expected y of the GPU module's polynomial blobs is a Horner value / a sum of a few powers: the same from the
    blob's 4096 values"""
    d, index = dom
    blobs, item_blob, zs, want = eval_items(257, d, index)
    seen = set()
    for i in range(64):
        if item_blob[i] in (0, 1):
            assert px.eval_form(blobs[item_blob[i]], zs[i], d, index) == want[i], i
            seen.add((item_blob[i], zs[i] in index))
    assert seen >= {(0, False), (1, False), (1, True)}   # both polynomials off the domain, one inside it too


def test_set_factors_are_the_host_replays(roots, host):
    host.hs_recover_set_factors.restype = None
    raw = rx.le32(roots)
    for held in recover_sets():
        zd, zi = C.create_string_buffer(128 * 32), C.create_string_buffer(128 * 32)
        host.hs_recover_set_factors(zd, zi, (C.c_uint32 * 4)(*px.mask_words(held)), raw, rx.le32([px.SEVEN64]))
        want = px.set_factors(held, roots)
        assert rx.from_le32(zd, 128) == want[0] and rx.from_le32(zi, 128) == want[1]


def test_gpu_module_items_against_the_host_replays_of_the_evaluation_kernels(dom, host):
    """four items of the GPU module's n = 7 launch -- z = 0 on the polynomial of degree 7, z = w_1 on the one of degree
    4095, z = w_4095 and z = w_2 + 1 on blobs with one non-zero leaf -- through hs_fr29_eval (k_eval_barycentric) and
    hs_fr29_eval_tree_bytes (k_eval_tree, both forms)"""
    d, index = dom
    blobs, item_blob, zs, want = eval_items(7, d, index)
    mont = lambda vals: b"".join((v * R256 % R).to_bytes(32, "little") for v in vals)
    roots_b = mont(d)
    host.hs_fr29_eval.restype = C.c_int
    host.hs_fr29_eval_tree_bytes.restype = None
    for i in (0, 1, 3, 4):
        blob, z = blobs[item_blob[i]], zs[i]
        y, di = C.create_string_buffer(32), C.create_string_buffer(4096 * 32)
        hit = host.hs_fr29_eval(y, di, mont(blob), mont([z]), roots_b)
        assert hit == index.get(z, -1)
        assert int.from_bytes(y.raw, "little") == want[i] * R256 % R
        for log_per in (6, 4):
            y2, bad = C.create_string_buffer(32), (C.c_uint32 * 1)(0)
            host.hs_fr29_eval_tree_bytes(y2, bad, b"".join(v.to_bytes(32, "big") for v in blob), mont([z]), roots_b, log_per)
            assert int.from_bytes(y2.raw, "little") == want[i] * R256 % R and bad[0] == 0
    assert zs[0] == 0 and item_blob[:2] == [0, 1] and index.get(zs[1]) == 1 and index.get(zs[3]) == 4095 and zs[4] == (d[2] + 1) % R and want[4] != 0


# ---- the shim ----

@pytest.fixture(scope="module")
def poly_shim_path():
    if not os.path.exists(POLY_SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "-j", "8", "libpoly_shim.so"])
    return POLY_SHIM_SO


def test_poly_shim_builds_and_exports_what_the_gpu_module_binds(poly_shim_path):
    names = _defined(poly_shim_path)
    for fn in POLY_FUNCTIONS:
        assert fn in names, fn
    assert sorted(s for s in names if s.startswith("ps_")) == sorted(POLY_FUNCTIONS)
    # linked with the product's objects, without its version script: the stage functions it calls are the product's
    assert "verify_blob_kzg_proof_batch" in names
    assert any("fr_ntt_batch" in s for s in names) and any("eval_quotient_batch_device" in s for s in names)


def test_make_all_builds_the_poly_shim():
    with open(os.path.join(PKG, "Makefile")) as f:
        text = f.read()
    all_line = next(line for line in text.splitlines() if line.startswith("all:"))
    assert "libpoly_shim.so" in all_line.split()
    rule = next(line for line in text.splitlines() if line.startswith("libpoly_shim.so:"))
    assert "$(OBJS)" in rule
    clean = text.split("\nclean:")[1]
    assert "libpoly_shim.so" in clean and "csrc/poly_shim.d" in text.split("-include")[-1]


def test_the_poly_shim_stays_out_of_the_product():
    _product_exports_are_the_map()   # the export list is exactly exports.map (and holds no ss_*)
    prod = _defined(os.path.join(PKG, "libckzg_hip.so"))
    assert not [s for s in prod if s.startswith("ps_")]
    assert not [n for n in declared_symbols() if n not in prod]   # (tests/test_abi_exports.py: every declared symbol)
