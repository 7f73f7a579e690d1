"""ckzg_hip_verify_blob_kzg_proof_batch_groups without a GPU: the symbol is declared and exported, a settings struct
without GPU state gives C_KZG_ERROR (no CPU fallback), the binding checks its arguments, and the segmented scalar
arithmetic of verify.hip (k_blob_group_scalars, k_blob_group_ysum) -- replayed on the host over the index maps the
product builds (csrc/blob_groups_plan.hpp, through libhost_shim.so) -- gives, group by group, the two sums whose
pairing check is the oracle's verdict for that group."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

import rlc_expect as rx
from conftest import ROOT, SHIM_SO
from kzg_ctypes import HIP_SO, Kzg, KzgError, KZGSettings, TRUSTED_SETUP
from test_abi_exports import declared_symbols

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NAME = "ckzg_hip_verify_blob_kzg_proof_batch_groups"


def test_symbol_declared_and_exported():
    assert NAME in declared_symbols()
    assert "    %s;\n" % NAME in open(os.path.join(ROOT, "c-kzg-4844_amd", "exports.map")).read()
    assert hasattr(C.CDLL(HIP_SO), NAME)


def test_zeroed_settings_give_error_and_no_cpu_fallback():
    f = getattr(C.CDLL(HIP_SO), NAME)
    f.restype = C.c_int
    s = KZGSettings()
    ok, st = (C.c_bool * 2)(), (C.c_uint8 * 2)()
    start = (C.c_uint64 * 3)(0, 1, 2)
    assert f(ok, st, bytes(2 * 131072), bytes(96), bytes(96), start, C.c_uint64(2), C.byref(s)) == 2
    assert f(None, None, None, None, None, None, C.c_uint64(0), C.byref(s)) == 2


def test_binding_checks_its_arguments():
    api = Kzg.__new__(Kzg)   # no library: every check below fails before a call is made
    blob, p48 = bytes(131072), bytes(48)
    for groups in ([([blob], [p48])],                     # not three lists
                   [([blob], [p48, p48], [p48])],         # list lengths
                   [([blob, blob], [p48, p48], [p48])],
                   [([blob[:-1]], [p48], [p48])],         # a short blob
                   [([blob], [p48[:-1]], [p48])],         # a short commitment
                   [([blob], [p48], [p48 + b"0"])],       # a long proof
                   [([blob], [p48], [p48]), ([blob + b"0"], [p48], [p48])]):   # the second group
        with pytest.raises(KzgError):
            api.verify_blob_kzg_proof_batch_groups(groups)


# ---- the replay ----

@pytest.fixture(scope="module")
def h():
    if not os.path.exists(SHIM_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-kzg-4844_amd"), "csrc/libhost_shim.so"])
    lib = C.CDLL(SHIM_SO)
    assert hasattr(lib, "hs_blob_groups_replay")
    lib.hs_blob_groups_replay.restype = C.c_long
    return lib


def _limbs(v):
    return (C.c_uint32 * 8)(*[(v >> (32 * i)) & 0xffffffff for i in range(8)])


def _g1(h, b48):
    """compressed point -> Jacobian (Z = 1), in the shim's representation"""
    aff = C.create_string_buffer(96)
    assert h.hs_g1_uncompress(aff, b48) == 0
    if aff.raw == bytes(96):
        return bytes(144)
    gen = C.create_string_buffer(144)
    h.hs_g1_generator(gen)
    return aff.raw + gen.raw[96:]


def _g2(h, b96):
    aff = C.create_string_buffer(192)
    assert h.hs_g2_uncompress(aff, b96) == 0
    gen = C.create_string_buffer(288)
    h.hs_g2_generator(gen)
    return aff.raw + gen.raw[192:]


def _lincomb(h, pts, scalars):
    acc = bytes(144)
    for p, k in zip(pts, scalars):
        if k == 0 or p == bytes(144):
            continue
        t = C.create_string_buffer(144)
        h.hs_g1_mul(t, p, _limbs(k), 255)
        out = C.create_string_buffer(144)
        h.hs_g1_add_jac(out, acc, t.raw)
        acc = out.raw
    return acc


def _material(oracle):
    """(blob, commitment, blob proof, z, y) of three blobs, everything from the oracle"""
    out = []
    for b in range(3):
        blob = b"".join(b"\x00" + hashlib.sha256(b"blobgroups%d/%d" % (b, j)).digest()[:31] for j in range(4096))
        cm = oracle.blob_to_kzg_commitment(blob)
        z = oracle.compute_challenge(blob, cm)
        _, y = oracle.compute_kzg_proof(blob, z)
        out.append((blob, cm, oracle.compute_blob_kzg_proof(blob, cm), int.from_bytes(z, "big"), int.from_bytes(y, "big")))
    return out


def _batch_challenge(group):
    """eip4844.c:597-680 over the group's slice; 0 for a group that needs none"""
    if len(group) < 2:
        return 0
    d = hashlib.sha256(b"RCKZGBATCH___V1_" + (4096).to_bytes(8, "big") + len(group).to_bytes(8, "big"))
    for _, cm, proof, z, y in group:
        d.update(cm + z.to_bytes(32, "big") + y.to_bytes(32, "big") + proof)
    return int.from_bytes(d.digest(), "big") % R


def test_host_replay_of_the_segmented_arithmetic_matches_the_oracle(h, oracle):
    mat = _material(oracle)

    def swapped(i, j):   # blob i with blob j's proof (z and y are functions of blob and commitment: unchanged)
        return mat[i][:2] + (mat[j][2],) + mat[i][3:]

    # three valid blobs, an empty group, a group of one, two blobs with their proofs swapped, a blob appearing twice
    groups = [[mat[0], mat[1], mat[2]], [], [mat[1]], [swapped(0, 1), swapped(1, 0)], [mat[2], mat[0], mat[2], mat[1]]]
    want = [oracle.verify_blob_kzg_proof_batch(*[[t[k] for t in g] for k in range(3)]) for g in groups]
    assert want == [True, True, True, False, True]
    flat = [t for g in groups for t in g]
    n, G = len(flat), len(groups)
    start = [0]
    for g in groups:
        start.append(start[-1] + len(g))
    rs = [_batch_challenge(g) for g in groups]
    le = lambda vals: b"".join(v.to_bytes(32, "little") for v in vals)
    lines = open(TRUSTED_SETUP).read().split()
    assert lines[0] == "4096" and lines[1] == "65"
    g2 = lines[2 + 4096:2 + 4096 + 65]
    gen = C.create_string_buffer(144)
    h.hs_g1_generator(gen)
    pool = [_g1(h, t[1]) for t in flat] + [_g1(h, t[2]) for t in flat] + [gen.raw]
    g2_gen, g2_s = _g2(h, bytes.fromhex(g2[0])), _g2(h, bytes.fromhex(g2[1]))
    for quad_max in (8192, 0):   # both paddings of the jobs: 8 terms and 32
        cap = 4096
        sc = (C.c_uint32 * (cap * 8))()
        src = (C.c_uint32 * cap)()
        part_off = (C.c_uint32 * (2 * G + 1))()
        info = (C.c_uint32 * 2)()
        total = h.hs_blob_groups_replay(sc, src, part_off, info, C.c_size_t(cap), (C.c_uint64 * (G + 1))(*start), C.c_size_t(G),
                                        le(t[3] for t in flat), le(t[4] for t in flat), le(rs), C.c_size_t(quad_max))
        per = 8 if quad_max else 32
        assert total > 0 and total % 64 == 0 and info[0] == total and info[1] == (1 if quad_max else 0)
        scal = [sum(sc[8 * t + i] << (32 * i) for i in range(8)) for t in range(total)]
        assert all(src[t] == 0xffffffff and scal[t] == 0 for t in range(part_off[2 * G] * per, total))
        # every scalar is the integer the layout of blob_groups_plan.hpp puts there: a verdict cannot tell r^i from
        # another weight that lands consistently on item i's commitment, proof and y
        rx.check_terms(src[:total], scal, part_off[:],
                       rx.blob_group_terms([len(g) for g in groups], [t[3] for t in flat], [t[4] for t in flat], rs, per))
        got = []
        for g in range(G):
            sums = []
            for job, real in ((2 * g, 2 * len(groups[g]) + 1), (2 * g + 1, len(groups[g]))):
                lo, hi = part_off[job] * per, part_off[job + 1] * per
                assert all(src[t] < len(pool) or (src[t] == 0xffffffff and scal[t] == 0) for t in range(lo, hi))
                terms = [t for t in range(lo, hi) if src[t] != 0xffffffff]
                assert len(terms) == (real if groups[g] else 0), (g, job, len(terms))
                sums.append(_lincomb(h, [pool[src[t]] for t in terms], [scal[t] for t in terms]))
            if not groups[g]:
                assert sums == [bytes(144)] * 2
                got.append(True)
            else:
                got.append(h.hs_pairings_verify(sums[0], g2_gen, sums[1], g2_s) == 1)
        assert got == want, (quad_max, got)


@pytest.mark.parametrize("quad_max", [8192, 0])
def test_host_replay_weights_are_the_integers(h, quad_max):
    """the group sizes and challenges of tests/test_gpu_rlc_stages.py (a group's r = 0, another's = 1), term by term"""
    import random
    sizes = rx.GROUP_SIZES
    G, N = len(sizes), sum(sizes)
    rnd = random.Random(99 + quad_max)
    z = [rnd.randrange(R) for _ in range(N)]
    y = [rnd.randrange(R) for _ in range(N)]
    z[0], z[70], y[1], y[71] = 0, R - 1, 0, R - 1
    rs = rx.group_challenges(77 + quad_max)
    start = [sum(sizes[:g]) for g in range(G + 1)]
    cap = 4096
    sc = (C.c_uint32 * (cap * 8))()
    src = (C.c_uint32 * cap)()
    part_off = (C.c_uint32 * (2 * G + 1))()
    info = (C.c_uint32 * 2)()
    total = h.hs_blob_groups_replay(sc, src, part_off, info, C.c_size_t(cap), (C.c_uint64 * (G + 1))(*start), C.c_size_t(G),
                                    rx.le32(z), rx.le32(y), rx.le32(rs), C.c_size_t(quad_max))
    want = rx.blob_group_terms(sizes, z, y, rs, 8 if quad_max else 32)
    assert total == len(want[0]) and info[0] == total
    rx.check_terms(src[:total], rx.from_le32(sc, total), part_off[:], want)
