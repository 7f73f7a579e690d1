"""Runs under LD_PRELOAD=failalloc.so (tests/test_gpu_recover_rows_alloc.py starts it): every device / page-locked
allocation, then every stream and event creation, of ckzg_hip_recover_cells_and_kzg_proofs_rows is made to fail in
turn, once and (for allocations) from then on.  What must hold each time: the call returns C_KZG_MALLOC (allocations)
or C_KZG_ERROR / C_KZG_MALLOC (streams, events) -- or its normal result, where nothing it needed failed --, never a
crash; no device memory is kept; the same call right after on the same settings gives the right rows.  The call has
twelve rows over five sets of cells, a row of 63 cells and a row with a non-canonical field element among them.
Prints one JSON line."""
import ctypes as C
import json
import random

from walk import C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC, R, fr, load, problems, report, walk

k0 = load()
rnd = random.Random(5)
full = []
for i in range(2):
    blob = b"".join(fr(rnd.randrange(R)) for _ in range(4096))
    full.append(k0.compute_cells_and_kzg_proofs(blob))
k0.close()
NR = 12
SETS = [list(range(0, 128, 2)), list(range(64, 128)), sorted(rnd.sample(range(128), 70)), sorted(rnd.sample(range(128), 127)),
        list(range(128))]
rows = [[list(SETS[(3 * r) % 5]), [full[r % 2][0][c] for c in SETS[(3 * r) % 5]]] for r in range(NR)]
rows[4] = [list(range(63)), [full[0][0][c] for c in range(63)]]                          # too few cells: invalid
rows[9][1][3] = rows[9][1][3][:32] + R.to_bytes(32, "big") + rows[9][1][3][64:]          # a field element >= r: invalid
EXPECT_ST = [int(r in (4, 9)) for r in range(NR)]
CELLS, PROOFS = 128 * 2048, 128 * 48
START = [0]
for idx, _ in rows:
    START.append(START[-1] + len(idx))
FLAT_IDX = [i for idx, _ in rows for i in idx]
ARGS = [(C.c_uint64 * len(FLAT_IDX))(*FLAT_IDX), b"".join(c for _, cells in rows for c in cells), (C.c_uint64 * (NR + 1))(*START)]
GOOD = [r for r in range(NR) if not EXPECT_ST[r]]
EXPECT_OUT = [b"".join(full[r % 2][0]) + b"".join(full[r % 2][1]) for r in range(NR)]


def call(k):
    rc = C.create_string_buffer(NR * CELLS)
    rp = C.create_string_buffer(NR * PROOFS)
    st = (C.c_uint8 * NR)()
    f = k.lib.ckzg_hip_recover_cells_and_kzg_proofs_rows
    f.restype = C.c_int
    ret = f(rc, rp, st, ARGS[0], ARGS[1], ARGS[2], C.c_uint64(NR), k.sp)
    if ret not in (0, C_KZG_BADARGS):
        return ret, None, None
    craw, praw = rc.raw, rp.raw
    # (the output of the row with the non-canonical element is unspecified, the invalid row's is not written)
    return ret, [craw[r * CELLS:(r + 1) * CELLS] + praw[r * PROOFS:(r + 1) * PROOFS] for r in GOOD], bytes(st)


def want_ok(key, want):
    if want[0] != C_KZG_BADARGS or want[1] != [EXPECT_OUT[r] for r in GOOD] or list(want[2]) != EXPECT_ST:
        return "%s: unarmed call gave %d, status %s, rows right: %s" % (
            key, want[0], want[2] and list(want[2]), want[1] and [a == EXPECT_OUT[r] for a, r in zip(want[1], GOOD)])
    return None


walk(0, (C_KZG_MALLOC,), (0, 1), "allocations", call, want_ok, noun="rows")
walk(1, (C_KZG_ERROR, C_KZG_MALLOC), (0,), "streams_events", call, want_ok, noun="rows")
print(json.dumps({"report": report, "problems": problems}))
