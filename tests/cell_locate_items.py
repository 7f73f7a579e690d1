"""What the tests of ckzg_hip_verify_cell_kzg_proof_batch_locate share: the consensus vectors of
verify_cell_kzg_proof_batch flattened into single cells, built items of each kind, and the expected verdict of an item
-- the CPU oracle's verify_cell_kzg_proof_batch on that item alone, computed once per distinct item."""
import hashlib

import g1_points as GP
from kzg_ctypes import KzgError, TRUSTED_SETUP

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BADARGS = 1
NOT_G1 = GP.by_label("Q+T11").data


def ceil_log2(m):
    return (m - 1).bit_length()


def spec_items():
    """(commitment, cell_index, cell, proof, vector's expected value, vector's name) for every cell of every
    well-formed verify_cell_kzg_proof_batch vector, in the vectors' order"""
    from test_gpu_cell_groups import _spec_groups
    items = []
    for (c, i, x, p), exp, name in _spec_groups()[0]:
        items.extend((c[k], i[k], x[k], p[k], exp, name) for k in range(len(x)))
    return items


_VERDICTS = {}


def verdict(oracle, item):
    """(ok, status) of the oracle's verify_cell_kzg_proof_batch on the one item; one oracle call per distinct item"""
    key = tuple(item[:4])
    if key not in _VERDICTS:
        try:
            _VERDICTS[key] = (oracle.verify_cell_kzg_proof_batch([item[0]], [item[1]], [item[2]], [item[3]]), 0)
        except KzgError:
            _VERDICTS[key] = (False, BADARGS)
    return _VERDICTS[key]


def flip_low_bit(cell, element):
    """the lowest bit of one field element flipped; the element must stay canonical"""
    b = bytearray(cell)
    b[32 * element + 31] ^= 1
    assert int.from_bytes(b[32 * element:32 * element + 32], "big") < R
    return bytes(b)


def non_canonical(cell, element):
    return cell[:32 * element] + R.to_bytes(32, "big") + cell[32 * element + 32:]


def digest(items):
    """the chunk's two-level challenge digest with hashlib"""
    leaves = b"".join(hashlib.sha256(b"CKZGHIPCELLLEAF_" + t[0] + int(t[1]).to_bytes(8, "big") + t[2] + t[3]).digest() for t in items)
    return hashlib.sha256(b"CKZGHIPCELLROOT_" + (4096).to_bytes(8, "big") + len(items).to_bytes(8, "big") + leaves).digest()


def setup_lines():
    lines = open(TRUSTED_SETUP).read().split()
    assert lines[0] == "4096" and lines[1] == "65"
    return lines


def setup_mono64():
    """g1_values_monomial[0..63], compressed, as the setup file has them"""
    lines = setup_lines()
    return b"".join(bytes.fromhex(v) for v in lines[2 + 4096 + 65:2 + 4096 + 65 + 64])


def setup_s64_g2():
    """[s^64]_2, compressed"""
    return bytes.fromhex(setup_lines()[2 + 4096 + 64])
