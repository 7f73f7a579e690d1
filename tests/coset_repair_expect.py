"""The model of the repair planning of ckzg_hip_repair_cosets_and_kzg_proofs_rows in plain Python: the verdict of a row
from its flags, which rows go to the locate pass and as which flat items, which rows are recovered a second time from
which of the caller's cosets, where those rows land, and the final verdicts.  The product's version is
csrc/coset_repair_plan.hpp (tests/test_coset_repair_cpu.py compares them through libhost_shim.so)."""
OK, INCONSISTENT, MISMATCH, REPAIRED, UNRECOVERABLE, INVALID = range(6)
NAMES = ["OK", "INCONSISTENT", "MISMATCH", "REPAIRED", "UNRECOVERABLE", "INVALID"]


def first_verdict(invalid, high, mismatch):
    """INVALID before INCONSISTENT before MISMATCH before OK"""
    if invalid:
        return INVALID
    if high:
        return INCONSISTENT
    return MISMATCH if mismatch else OK


def plan(status, high1, mismatch1, row_start, e, with_proofs=False, item_ok=None, high2=None, mismatch2=None):
    """one shard over all rows.  item_ok: the locate pass's answer for every coset of the caller's flat list (only those
    of located rows are looked at); high2 / mismatch2: the second pass's flags per caller row"""
    nr, need = len(status), (8192 >> e) // 2
    verdict = [first_verdict(status[r] != 0, high1[r], mismatch1[r]) for r in range(nr)]
    coset_ok = []
    for r in range(nr):
        coset_ok += [verdict[r] == OK] * (row_start[r + 1] - row_start[r])
    out = dict(loc_rows=[], item_src=[], item_row=[], out_row=[], start2=[0], src2=[], lost=[])
    if with_proofs:
        for r in range(nr):
            if verdict[r] not in (INCONSISTENT, MISMATCH):
                continue
            held = list(range(row_start[r], row_start[r + 1]))
            out["loc_rows"].append(r)
            out["item_src"] += held
            out["item_row"] += [r] * len(held)
            good = [i for i in held if item_ok[i]]
            for i in held:
                coset_ok[i] = bool(item_ok[i])
            if len(good) < need:
                out["lost"].append(r)
                verdict[r] = UNRECOVERABLE
                continue
            out["out_row"].append(r)
            out["src2"] += good
            out["start2"].append(len(out["src2"]))
            verdict[r] = UNRECOVERABLE if (high2[r] or mismatch2[r]) else REPAIRED
    out["verdict"], out["coset_ok"] = verdict, coset_ok
    return out
