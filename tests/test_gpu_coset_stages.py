"""The column sum of the coset openings (g1_fft.hip: coset_colsum_enqueue, k_coset_colsum) read off the device and
compared with integers.  ckzg_hip_compute_coset_kzg_proofs_batch reaches it with the products of honest blobs, which
never meet an equal or an opposite operand; here every point is a_i * G with a chosen small a_i (tests/g1_expect.py),
in XYZZ form with a z that is not one, so the expected value of every output is one integer mod r.

tests/native/coset_shim.hip (libcoset_shim.so: its entry file linked with the product's own object files) runs the
stage on rows of 8192 points.  The order of the additions is replayed here (one pass up to 8 columns; above, 8 columns
into each of l / 8 parts, then the parts), and the chosen scalars make the running sum meet an equal operand (a
doubling), an opposite operand (a cancellation), the identity as operand and the identity as running sum at chosen
columns -- in both passes where there are two.  The replay asserts that they do."""
import ctypes as C
import os
import random
import subprocess

import pytest

import g1_expect as gx
from conftest import ROOT, ORACLE_SO

pytestmark = pytest.mark.gpu
R = gx.R
COSET_SHIM_SO = os.path.join(ROOT, "c-kzg-4844_amd", "libcoset_shim.so")
RADIX = 8   # g1_fft_plan.hpp: COSET_COLSUM_RADIX (tests/test_coset_openings_cpu.py pins it)


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(COSET_SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "-j", "8", "libcoset_shim.so"])
    lib = C.CDLL(COSET_SHIM_SO)
    lib.cos_colsum.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def src():
    if not os.path.exists(ORACLE_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    return gx.G1Source(C.CDLL(ORACLE_SO))


def chains(l):
    """the passes of the sum over l columns: a list of passes, each a list of chains of column indices; a chain's sum
    lands in its first column"""
    parts = l // RADIX if l > RADIX else 1
    if parts == 1:
        return [[list(range(l))]]
    return [[list(range(p, l, parts)) for p in range(parts)], [list(range(parts))]]


def replay(l, col):
    """col[i]: the scalar in column i at one position.  Returns (sum, events): events are (pass, chain, step, kind)
    with kind in load (identity running sum), skip (identity operand), double, cancel"""
    val, events = list(col), []
    for ps, chs in enumerate(chains(l)):
        for ch_no, ch in enumerate(chs):
            acc = val[ch[0]] % R
            for step, i in enumerate(ch[1:], 1):
                b = val[i] % R
                if b == 0:
                    events.append((ps, ch_no, step, "skip"))
                elif acc == 0:
                    events.append((ps, ch_no, step, "load"))
                elif acc == b:
                    events.append((ps, ch_no, step, "double"))
                elif (acc + b) % R == 0:
                    events.append((ps, ch_no, step, "cancel"))
                acc = (acc + b) % R
            val[ch[0]] = acc
    return val[0], events


def chosen_column(l, kind, rnd):
    """l scalars whose sum meets the events of `kind` in every pass"""
    col = [rnd.choice([1, 2, 3, 4, 5, -1, -2, -3]) for _ in range(l)]
    passes = chains(l)
    first = passes[0][0]                      # the first chain of the first pass: steps 1, 2, 3 are chosen
    if kind == "double":
        col[first[0]], col[first[1]] = 3, 3               # 3 + 3
    elif kind == "cancel":
        for i, v in zip(first, (4, -4, 0, 2)):            # 4 - 4, then the identity twice, then a load
            col[i] = v
    elif kind == "identity":
        col[first[0]], col[first[1]] = 0, 0               # the identity plus the identity
    if len(passes) == 2:
        # the parts' totals: chain p of the first pass ends in its last column, which sets the total
        parts = len(passes[0])
        want = {"double": [5, 5], "cancel": [6, -6, 0, 7], "identity": [0, 0, 0, 1]}[kind]
        for p, tot in enumerate(want[:parts]):
            ch = passes[0][p]
            col[ch[-1]] = tot - sum(col[i] for i in ch[:-1])
    return col


@pytest.mark.parametrize("e,rows", [(1, 1), (3, 2), (6, 1)])
def test_column_sum_on_chosen_points(shim, src, e, rows):
    l, w = 1 << e, 8192 >> e
    rnd = random.Random(e)
    kinds = ["double", "cancel", "identity", None]
    scal = [[None] * w for _ in range(rows)]
    seen = set()
    for b in range(rows):
        for t in range(w):
            kind = kinds[(t + b) % 4] if t % 64 in (0, 1, 2, 3, 63) or t >= w - 4 else None   # first and last lanes of a wave, the last positions
            col = chosen_column(l, kind, rnd) if kind else [rnd.choice([0, 1, 2, 3, -1, -2, -3]) for _ in range(l)]
            scal[b][t] = col
            for ps, _, _, k in replay(l, col)[1]:
                seen.add((ps, k))
    npass = len(chains(l))
    if l > 2:   # (two columns are one addition: no identity after a cancellation)
        assert seen >= {(ps, k) for ps in range(npass) for k in ("load", "skip", "double", "cancel")}, seen
    else:
        assert seen >= {(0, k) for k in ("skip", "double", "cancel")}, seen
    buf = bytearray(rows * 8192 * 192)
    for b in range(rows):
        for i in range(l):
            for t in range(w):
                a = scal[b][t][i]
                z = 2 + (3 * i + t + b) % 5
                o = ((b * 8192) + i * w + t) * 192
                buf[o:o + 192] = gx.xyzz_raw(src.point(a) if a % R else gx.INF, z)
    data = (C.c_uint8 * len(buf)).from_buffer(buf)
    rc = C.c_int(-1)
    assert shim.cos_colsum(data, C.c_size_t(rows), e, C.byref(rc)) == 0 and rc.value == 0
    for b in range(rows):
        for t in range(w):
            want, _ = replay(l, scal[b][t])
            assert want == sum(scal[b][t]) % R
            o = (b * 8192 + t) * 192
            assert gx.xyzz_is(bytes(buf[o:o + 192]), src.raw(want)), (b, t, scal[b][t])


def test_the_shim_refuses_what_the_stage_does_not_serve(shim):
    rc = C.c_int(-1)
    buf = (C.c_uint8 * 192)()
    for rows, e in ((0, 3), (5, 3), (1, 7), (1, -1)):
        assert shim.cos_colsum(buf, C.c_size_t(rows), e, C.byref(rc)) == 9998
    assert rc.value == -1
