"""What can be said about the device test shim (tests/native/dev_shim.hip) and the generated inline-asm product
without a GPU: libdev_shim.so cross-compiles for gfx950 and exports every ds_plain_* / ds_asm_* pair that
tests/test_gpu_dev_arith.py and tests/test_gpu_fp30.py bind and the ds_dev_* functions of tests/test_gpu_fields.py, both forms and the host shim carry the same lists of F28 and F30 instantiations, and the
committed csrc/fp28_asm_cols.inc is byte for byte what tools/gen_fp28_asm.py emits."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import ROOT, SHIM_SO
from test_gpu_dev_arith import DEV_FUNCTIONS, DEV_SHIM_SO, FORMS, SHIM_FUNCTIONS
from test_gpu_fp30 import SHIM_FUNCTIONS_30

PKG = os.path.join(ROOT, "c-kzg-4844_amd")


@pytest.fixture(scope="module")
def dev_shim_path():
    if not os.path.exists(DEV_SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "-j", "2", "libdev_shim.so"])
    return DEV_SHIM_SO


def test_dev_shim_builds_and_exports_both_forms(dev_shim_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", dev_shim_path], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for form in FORMS:
        for fn in SHIM_FUNCTIONS + SHIM_FUNCTIONS_30:
            assert "ds_%s_%s" % (form, fn) in names, (form, fn)
    for fn in DEV_FUNCTIONS:               # tests/native/dev_shim_fields.hip: one plain build
        assert fn in names, fn
    # the test aid stays out of the product
    if not os.path.exists(os.path.join(PKG, "libckzg_hip.so")):
        subprocess.check_call(["make", "-C", PKG, "-j", "4", "libckzg_hip.so"])
    prod = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libckzg_hip.so")], text=True)
    assert "ds_plain_" not in prod and "ds_asm_" not in prod and "ds_dev_" not in prod


def test_all_shims_list_the_same_instantiations(dev_shim_path):
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", PKG, "csrc/libhost_shim.so"])
    d, h = C.CDLL(dev_shim_path), C.CDLL(SHIM_SO)
    h.hs_f28_ops.restype = C.c_char_p
    want = h.hs_f28_ops()
    assert want
    for form in FORMS:
        fn = getattr(d, "ds_%s_f28_ops" % form)
        fn.restype = C.c_char_p
        assert fn() == want, form
    # and of F30 ones (f30_test_ops.hpp), which is the list the corpora of tests/fp30_expect.py are drawn for
    import fp30_expect as fx
    h.hs_f30_ops.restype = C.c_char_p
    want = h.hs_f30_ops()
    assert fx.parse_ops(want.decode()) == fx.REQUIRED_OPS
    for form in FORMS:
        fn = getattr(d, "ds_%s_f30_ops" % form)
        fn.restype = C.c_char_p
        assert fn() == want, form


def test_generated_asm_product_matches_its_generator():
    got = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_fp28_asm.py")])
    with open(os.path.join(PKG, "csrc", "fp28_asm_cols.inc"), "rb") as f:
        assert got == f.read()
