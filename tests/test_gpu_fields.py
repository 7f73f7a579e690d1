"""The other half of what only the device compiler builds -- Mont<Fp> / Mont<Fr> on the 32-bit CIOS (field.hpp: what
every Fr kernel and the whole pairing run), Fr29 with its called product fr29_mul_regs, the safegcd inversions with
their device-only lines, and the pairing tower of tower.hpp / pairing_dev.hpp with its out-of-line products -- fed the
corpora of tests/field_cases.py through tests/native/dev_shim_fields.hip (libdev_shim.so: ds_dev_field, one plain
build) and compared with the exact references that tests/test_field_corpora_cpu.py validates on the host: Python
integers, and the Python tower of tests/tower_ref.py.  No tolerance anywhere.

Geometry.  One thread per item; lanes past the end repeat the last item and store nothing.  Every list runs twice:
whole, in workgroups of 256, and its first 101 items in workgroups of 64, which leaves a wave with 37 live lanes.
After any non-zero return of a shim call every later test of the module fails at once without launching anything."""
import ctypes as C
import os
import subprocess

import pytest

import field_cases as fc
from conftest import ROOT, SHIM_SO
from test_gpu_dev_arith import DEV_SHIM_SO

pytestmark = pytest.mark.gpu


class FieldShim:
    """ds_dev_field of libdev_shim.so; remembers the first failed call and refuses every later one"""

    def __init__(self, lib):
        self.lib = lib
        self.dead = None
        lib.ds_dev_field_ops.restype = C.c_char_p
        self.ops = fc.parse_ops(lib.ds_dev_field_ops().decode())

    def run(self, name, items, count, block):
        if self.dead is not None:
            pytest.fail("an earlier shim call (%s) returned %d: nothing is launched any more" % self.dead)
        k = [n for n, _, _ in self.ops].index(name)
        _, widths, shared = self.ops[k]
        a, b, c, d = [(C.c_uint32 * len(buf))(*buf) for buf in fc.pack(items[:count], widths, shared)]
        out = (C.c_uint32 * (widths[0] * count))()
        rc = self.lib.ds_dev_field(k, out, a, b, c, d, count, block)
        if rc != 0:
            self.dead = (name, rc)
            pytest.fail("ds_dev_field(%s) returned %d" % (name, rc))
        return out, widths[0]

    def both_geometries(self, name, items, wants):
        """-> the whole list's output"""
        whole = None
        for count, block in ((len(items), 256), (min(fc.SUBSET_LEN, len(items)), 64)):
            out, wo = self.run(name, items, count, block)
            fc.check(name, wants, out, wo, count)
            whole = whole or out
        return whole


@pytest.fixture(scope="module")
def env():
    pkg = os.path.join(ROOT, "c-kzg-4844_amd")
    if not os.path.exists(DEV_SHIM_SO):
        subprocess.check_call(["make", "-C", pkg, "-j", "3", "libdev_shim.so"])
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", pkg, "csrc/libhost_shim.so"])
    return C.CDLL(SHIM_SO), FieldShim(C.CDLL(DEV_SHIM_SO))


def test_the_list_is_the_one_the_host_runs(env):
    h, shim = env
    h.hs_field_ops.restype = C.c_char_p
    assert shim.lib.ds_dev_field_ops() == h.hs_field_ops()
    names = [n for n, _, _ in shim.ops]
    for want in fc.REQUIRED_OPS:
        assert want in names, want
    assert sorted(names) == sorted(fc.REQUIRED_OPS)        # nothing is listed that no test below runs


@pytest.mark.parametrize("name", [n for n in fc.REQUIRED_OPS if n not in fc.PAIRING_OPS])
def test_device_form_on_the_corpora(env, name):
    _, shim = env
    items, wants = fc.cached_corpus(name)
    shim.both_geometries(name, items, wants)


def test_miller_product_matches_host_and_the_python_tower(env):
    """byte for byte host_pairing.hpp's value, and -- by the Python tower alone -- final_exp(miller([a]P, [b]Q)) ==
    final_exp(miller(P, Q))^(a b).  One wave mixes infinite and finite G1 arguments in both slots"""
    h, shim = env
    items, wants, extra = fc.pairing_corpus("miller_product_tables", h)
    out = shim.both_geometries("miller_product_tables", items, wants)
    fc.check_miller_relation([list(out[144 * i:144 * (i + 1)]) for i in range(len(items))], extra)


def test_two_pair_verdicts(env):
    h, shim = env
    items, wants, _ = fc.pairing_corpus("pairing_product_is_one", h)
    assert len(items) == 37
    shim.both_geometries("pairing_product_is_one", items, wants)
