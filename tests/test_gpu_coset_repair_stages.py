"""The device stages of ckzg_hip_repair_cosets_and_kzg_proofs_rows (csrc/coset_repair.hip) read off the GPU through
libcoset_repair_shim.so (tests/native/coset_repair_shim.hip: the product's objects behind a C ABI): the degree flag of a
row on chosen coefficient patterns, the recoding of a row's blob half and its commitment against the oracle's
blob_to_kzg_commitment, the comparison of commitments.  Every written buffer has a guard region on both sides."""
import ctypes as C
import os
import random
import subprocess

import pytest

from conftest import ORACLE_SO, ROOT
from test_gpu_g1_stages import edge_scalars

pytestmark = pytest.mark.gpu
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SHIM_SO = os.path.abspath(os.environ["CKZG_COSET_REPAIR_SHIM_SO"]) if os.environ.get("CKZG_COSET_REPAIR_SHIM_SO") else \
    os.path.join(ROOT, "c-kzg-4844_amd", "libcoset_repair_shim.so")
SZ = C.c_size_t
GUARD_BYTE = 0xa5
ROW = 8192


class Shim:
    """remembers the first failed call and refuses every later one"""

    def __init__(self, lib):
        self.lib, self.dead = lib, None
        self.guard = lib.crp_guard()

    def call(self, name, *args):
        if self.dead is not None:
            pytest.fail("an earlier shim call (%s) returned %d: nothing is launched any more" % self.dead)
        rc = C.c_int(-1)
        run = getattr(self.lib, name)(*args, C.byref(rc))
        if run != 0:
            self.dead = (name, run)
            pytest.fail("%s returned %d" % (name, run))
        return rc.value


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libcoset_repair_shim.so"])
    lib = C.CDLL(SHIM_SO)
    for fn in ("crp_high_degree", "crp_rows_commit", "crp_commit_compare"):
        getattr(lib, fn).restype = C.c_int
    lib.crp_guard.restype = C.c_size_t
    return Shim(lib)


def le_rows(rows):
    return b"".join(v.to_bytes(32, "little") for row in rows for v in row)


def guarded_words(shim, n):
    return C.create_string_buffer(bytes([GUARD_BYTE]) * (4 * (n + 2 * shim.guard)), 4 * (n + 2 * shim.guard))


def words_out(shim, buf, n):
    """the n words between the guards; the guards must be as they were"""
    g = 4 * shim.guard
    raw = buf.raw
    assert raw[:g] == bytes([GUARD_BYTE]) * g and raw[g + 4 * n:] == bytes([GUARD_BYTE]) * g, "a guard region was written"
    return [int.from_bytes(raw[g + 4 * i:g + 4 * i + 4], "little") for i in range(n)]


def test_high_degree_flags(shim):
    rnd = random.Random(4096)
    zero = [0] * ROW
    only = lambda at, v=1: [v if i == at else 0 for i in range(ROW)]
    low_full = [rnd.randrange(R) for _ in range(4096)] + [0] * 4096          # degree 4095 with every low coefficient set
    rows = [zero, only(4095), only(4096), only(8191), only(4096 + rnd.randrange(4096), R - 1), low_full,
            only(6000, 1 << 224),                                            # a single high limb
            [rnd.randrange(R) for _ in range(ROW)], only(4095, R - 1)]
    want = [0, 0, 1, 1, 1, 0, 1, 1, 0]
    flags = guarded_words(shim, len(rows))
    assert shim.call("crp_high_degree", flags, le_rows(rows), SZ(len(rows))) == 0
    assert words_out(shim, flags, len(rows)) == want
    # one row alone, and the flag of a row does not leak into its neighbours in either direction
    for rows, want in (([only(8191)], [1]), ([zero, only(4096), zero], [0, 1, 0]), ([only(8191), zero, only(4096)], [1, 0, 1])):
        flags = guarded_words(shim, len(rows))
        assert shim.call("crp_high_degree", flags, le_rows(rows), SZ(len(rows))) == 0
        assert words_out(shim, flags, len(rows)) == want


def setup_bases():
    """the 4096 compressed Lagrange points of the trusted setup in the order of the commitment table: bit-reversed"""
    lines = open(os.path.join(ROOT, "c-kzg-4844_amd", "data", "trusted_setup.txt")).read().split()
    assert lines[0] == "4096" and lines[1] == "65"
    pts = [bytes.fromhex(h) for h in lines[2:2 + 4096]]
    brp = lambda i: int(format(i, "012b")[::-1], 2)
    return b"".join(pts[brp(i)] for i in range(4096))


def test_rows_digits_and_commitment_against_the_oracle(shim, oracle):
    c = 4
    rnd = random.Random(7594)
    edge = edge_scalars(c, rnd)
    firsts = [[edge[(i + 5 * v) % len(edge)] if i % 3 == 0 else rnd.randrange(R) for i in range(4096)] for v in range(2)]
    firsts[0][0], firsts[0][1], firsts[0][4095] = 0, 1, R - 1
    firsts.append([0] * 4096)
    tail = lambda: [rnd.randrange(R) for _ in range(4096)]
    # rows 0 and 3 share their first half and differ in their second: the second half must not matter
    rows = [firsts[0] + tail(), firsts[1] + [R - 1] * 4096, firsts[2] + tail(), firsts[0] + [0] * 4096]
    which = [0, 1, 2, 0]
    want = [oracle.blob_to_kzg_commitment(b"".join(v.to_bytes(32, "big") for v in f)) for f in firsts]
    assert want[2] == b"\xc0" + bytes(47)
    g = shim.guard
    out = C.create_string_buffer(bytes([GUARD_BYTE]) * (48 * 4 + 2 * g), 48 * 4 + 2 * g)
    assert shim.call("crp_rows_commit", out, le_rows(rows), SZ(4), setup_bases(), c) == 0
    raw = out.raw
    assert raw[:g] == bytes([GUARD_BYTE]) * g and raw[g + 192:] == bytes([GUARD_BYTE]) * g, "a guard region was written"
    for r, b in enumerate(which):
        assert raw[g + 48 * r:g + 48 * r + 48] == want[b], "row %d" % r


def test_commit_compare(shim):
    rnd = random.Random(48)
    n = 300                                          # more than one workgroup
    got = [bytes(rnd.randrange(256) for _ in range(48)) for _ in range(n)]
    want = list(got)
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 0x80]) + b[at + 1:]
    want[0] = flip(want[0], 0)
    want[7] = flip(want[7], 47)
    want[255] = flip(want[255], 16)
    want[256] = flip(want[256], 31)
    want[299] = flip(flip(want[299], 0), 47)
    flags = guarded_words(shim, n)
    assert shim.call("crp_commit_compare", flags, b"".join(got), b"".join(want), SZ(n)) == 0
    assert words_out(shim, flags, n) == [1 if i in (0, 7, 255, 256, 299) else 0 for i in range(n)]
    flags = guarded_words(shim, 1)
    assert shim.call("crp_commit_compare", flags, got[3], got[3], SZ(1)) == 0
    assert words_out(shim, flags, 1) == [0]
