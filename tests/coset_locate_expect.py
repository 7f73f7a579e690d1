"""What ckzg_hip_verify_coset_kzg_proof_batch_locate adds to the models of tests/coset_verify_expect.py (the check of one
item, the index maps) and tests/cell_locate_expect.py (digits as scalars), as Python integers and hashlib
(tests/test_coset_locate_cpu.py, tests/test_gpu_coset_locate_stages.py, tests/test_gpu_coset_locate.py).  Nothing here
reads the library under test.

An item is (commitment 48, coset index, values 32 l, proof 48); l = 2^e values in the order of brp_roots_of_unity[c l ..]."""
import hashlib

import coset_verify_expect as V
from cell_locate_expect import digits_scalar   # noqa: F401  (the stage tests read digits through it)
from domain_expect import R, root_of_unity

BADARGS = 1
CHUNK_SLOTS = 1048576
CHUNK_ITEMS_MAX = 65536
MIN_SHARD = 64
# csrc/coset_locate_plan.hpp, restated: one wave per vector below WAVE_BELOW[e] items, LPV[e] lanes per vector from there on
WAVE_BELOW = [2048, 2048, 4096, 4096, 8192, 8192, 4096]
LPV = [4, 8, 8, 8, 8, 8, 16]


def ceil_log2(m):
    return (m - 1).bit_length()


def chunk_items(e):
    return min(CHUNK_ITEMS_MAX, CHUNK_SLOTS >> e)


def sum_lpv(e, items):
    return 64 if items < WAVE_BELOW[e] else LPV[e]


def switch_points(e):
    """the item counts at which the form of the sums changes"""
    return [WAVE_BELOW[e]]


def leaf(item, e, l_field=None):
    cm, c, ev, pf = item
    assert len(cm) == 48 and len(pf) == 48 and len(ev) == 32 << e
    l = (1 << e) if l_field is None else l_field
    return hashlib.sha256(b"CKZGHIPCOSETLEAF" + cm + l.to_bytes(8, "big") + int(c).to_bytes(8, "big") + ev + pf).digest()


def digest(items, e, l_field=None):
    """the chunk's two-level challenge digest; l_field: another number in the place of l, the bytes otherwise the same"""
    l = (1 << e) if l_field is None else l_field
    leaves = b"".join(leaf(t, e, l_field) for t in items)
    return hashlib.sha256(b"CKZGHIPCOSETROOT" + (4096).to_bytes(8, "big") + l.to_bytes(8, "big") + len(items).to_bytes(8, "big") +
                          leaves).digest()


def minus_interp(ys, c, e):
    """-a_k, k < l: what the digit kernel writes for an item with values ys on coset c (c < 8192 >> e)"""
    return [(-a) % R for a in V.interp_coeffs(ys, c, e)]


def clamp(c, e):
    """the coset the digit kernel looks up for an index that may be out of range"""
    return min(c, (8192 >> e) - 1)


def p1_log(a_commit, b_proof, ys, c, e, s):
    """the discrete logarithm of P1 = C - [I(s)]G + [x_c^l] proof for C = [a]G, proof = [b]G, bases [s^k]G"""
    i_s = sum(a * pow(s, k, R) for k, a in enumerate(V.interp_coeffs(ys, c, e))) % R
    xl = pow(root_of_unity(8192), V.shift_root(c, e), R)
    return (a_commit - i_s + xl * b_proof) % R


def checks_bound(nfalse, n):
    """the most host range checks a chunk of n items with nfalse false ones may cost"""
    return 1 + 2 * nfalse * ceil_log2(n)
