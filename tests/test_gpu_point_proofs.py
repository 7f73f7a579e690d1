"""ckzg_hip_verify_kzg_proof_batch: verify_kzg_proof over n independent items, one verdict per item, pairings on the
GPU (c-kzg-4844_amd/csrc/pairing.hip).  Every item must come out exactly as the single verify_kzg_proof call does:
the consensus-spec vectors in one call, special vectors at the wave edges, large batches of known verdicts against
single calls, invalid items next to valid ones, the shard split, concurrent callers; plus the kernels' resource gate."""
import ctypes as C
import importlib.util
import os
import random
import threading

import pytest

from golden_util import case_names, get_case
from kzg_ctypes import HIP_SO, Kzg

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = b"\xc0" + bytes(47)
BADARGS = 1


def _spec_items():
    """(commitment, z, y, proof, expected) for every verify_kzg_proof vector with well-formed inputs; expected is
    True / False, or None for a call that must fail with C_KZG_BADARGS"""
    items = []
    for name in case_names("verify_kzg_proof"):
        inp, exp = get_case("verify_kzg_proof", name)
        c, z, y, p = inp["commitment"], inp["z"], inp["y"], inp["proof"]
        if any(v is None for v in (c, z, y, p)) or len(c) != 48 or len(p) != 48 or len(z) != 32 or len(y) != 32:
            continue
        items.append((c, z, y, p, exp, name))
    return items


def _check(got, items):
    ok, st = got
    assert len(ok) == len(items) and len(st) == len(items)
    for i, it in enumerate(items):
        exp = it[4]
        if exp is None:
            assert st[i] == BADARGS and ok[i] is False, (i, it[5:])
        else:
            assert st[i] == 0 and ok[i] is exp, (i, it[5:], ok[i], exp)


def _run(api, items):
    return api.verify_kzg_proof_batch([t[0] for t in items], [t[1] for t in items], [t[2] for t in items],
                                      [t[3] for t in items])


@pytest.mark.gpu
def test_all_spec_vectors_in_one_call(hip):
    items = _spec_items()
    assert len(items) >= 100
    kinds = {t[4] for t in items}
    assert kinds == {True, False, None}
    # the zero polynomial / twos polynomial vectors have infinity as commitment or proof
    assert any(t[0] == INF or t[3] == INF for t in items if t[4] is True)
    _check(_run(hip, items), items)


@pytest.mark.gpu
def test_special_vectors_at_wave_edges(hip):
    items = _spec_items()
    special = [t for t in items if t[4] is None or t[0] == INF or t[3] == INF]
    plain = [t for t in items if not (t[4] is None or t[0] == INF or t[3] == INF)]
    assert special and plain
    rnd = random.Random(3)
    for n in (1, 2, 63, 64, 65, 1000):
        batch = [plain[rnd.randrange(len(plain))] for _ in range(n)]
        for j, lane in enumerate(sorted({0, 1, 31, 32, 63, 64, 65, n - 1})):
            if lane < n:
                batch[lane] = special[(j + n) % len(special)]
        _check(_run(hip, batch), batch)


def _fr(v):
    return (v % R).to_bytes(32, "big")


@pytest.fixture(scope="module")
def tuples(hip):
    """64 valid (commitment, z, y, proof) from compute_kzg_proof on random blobs; a quarter of the z on the
    evaluation domain (4096-th roots of unity)"""
    rnd = random.Random(7)
    w = pow(7, (R - 1) // 4096, R)
    out = []
    for i in range(64):
        blob = b"".join(_fr(rnd.randrange(R)) for _ in range(4096))
        c = hip.blob_to_kzg_commitment(blob)
        z = _fr(pow(w, rnd.randrange(4096), R)) if i % 4 == 0 else _fr(rnd.randrange(R))
        proof, y = hip.compute_kzg_proof(blob, z)
        out.append((c, z, y, proof))
    return out


def _mutants(tuples, n, seed):
    """n items of known verdict: valid tuples and mutants of them (y+1, z+1, another tuple's proof, proof and
    commitment swapped, infinity as proof)"""
    rnd = random.Random(seed)
    items = []
    for i in range(n):
        c, z, y, p = tuples[rnd.randrange(len(tuples))]
        kind = rnd.randrange(6)
        if kind == 1:
            y = _fr(int.from_bytes(y, "big") + 1)
        elif kind == 2:
            z = _fr(int.from_bytes(z, "big") + 1)
        elif kind == 3:
            o = tuples[rnd.randrange(len(tuples))][3]
            if o == p:
                kind = 0
            p = o
        elif kind == 4:
            c, p = p, c
        elif kind == 5:
            p = INF
        items.append((c, z, y, p, kind == 0, "mutant%d" % kind))
    return items


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4096, 65536, 65600])   # (65,600: two chunks of the call, the second a short one)
def test_large_batches_match_single_calls(hip, tuples, n):
    items = _mutants(tuples, n, n)
    ok, st = _run(hip, items)
    assert st == [0] * n
    assert ok == [t[4] for t in items]
    for i in random.Random(n + 1).sample(range(n), 256):
        c, z, y, p = items[i][:4]
        assert hip.verify_kzg_proof(c, z, y, p) is ok[i], i


@pytest.mark.gpu
def test_empty_and_one_invalid_item(hip, tuples):
    assert _run(hip, []) == ([], [])
    f = hip.lib.ckzg_hip_verify_kzg_proof_batch
    assert f(None, None, None, None, None, None, C.c_uint64(0), hip.sp) == 0
    items = _mutants(tuples, 200, 5)
    bad = list(items[77])
    bad[1] = R.to_bytes(32, "big")   # z not canonical
    bad[4] = None
    items[77] = tuple(bad)
    n = len(items)
    ok = (C.c_bool * n)()
    st = (C.c_uint8 * n)()
    j = lambda k: b"".join(t[k] for t in items)
    ret = f(ok, st, j(0), j(1), j(2), j(3), C.c_uint64(n), hip.sp)
    assert ret == BADARGS
    _check(([bool(v) for v in ok], list(st)), items)
    # status may be NULL
    ok2 = (C.c_bool * n)()
    assert f(ok2, None, j(0), j(1), j(2), j(3), C.c_uint64(n), hip.sp) == BADARGS
    assert list(ok2) == list(ok)


@pytest.mark.gpu
def test_shard_split_over_two_replicas(hip, tuples):
    items = _mutants(tuples, 3000, 9)
    want = _run(hip, items)
    api = Kzg(HIP_SO, "", precompute=0, options={"replicas": 2, "commit_wbits": 8, "proof_wbits": 6})
    try:
        assert _run(api, items) == want
    finally:
        api.close()
        # (options are process-wide: the defaults back for settings loaded later in the session)
        for k, v in ((b"replicas", 1), (b"commit_wbits", 10), (b"proof_wbits", 8)):
            api.lib.ckzg_hip_set_option(k, v)


@pytest.mark.gpu
def test_concurrent_callers(hip, tuples):
    batches = [_mutants(tuples, 100 + 150 * t, 100 + t) for t in range(8)]
    results = [None] * 8
    errors = []

    def work(t):
        try:
            results[t] = _run(hip, batches[t])
        except Exception as e:   # reported below
            errors.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors
    for t in range(8):
        _check(results[t], batches[t])


# measured by tools/kernel_resources.py on the build this file was written with (profiles/point_verify_resources.txt);
# the per-lane pairing runs one wave per SIMD by design (an Fp12 is 144 VGPRs)
BUDGET = {"k_pairing_check": {"vgpr": 512, "scratch": 11088},
          "k_point_lhs": {"vgpr": 254, "scratch": 5728}}


def test_point_verify_kernel_resources():
    if os.environ.get("CKZG_HIP_SO"):
        pytest.skip("sanitizer / variant build: the budget is the product's")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    table = {k.split(":", 1)[1]: v for k, v in m.collect().items()}
    for name, b in BUDGET.items():
        assert name in table, name
        assert table[name]["vgpr"] <= b["vgpr"], (name, table[name])
        assert table[name]["scratch"] <= b["scratch"], (name, table[name])
