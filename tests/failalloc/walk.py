"""What the drivers of this directory share (all but driver.py, whose walks are of another shape): the ctypes
declarations of failalloc.so, load() and walk() -- every device / page-locked allocation (class 0) or every stream and
event creation (class 1) of one call is made to fail in turn, once or from then on.  What must hold each time: the call
returns one of `allowed` -- or its normal result, where nothing it needed failed --, never a crash; no device memory is
kept; the same call right after on the same settings gives the unarmed result.  A driver keeps its data, its call()
and its own check of the unarmed result, and prints report and problems as one JSON line."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from kzg_ctypes import Kzg, HIP_SO  # noqa: E402

LIB = os.environ.get("CKZG_HIP_SO") or HIP_SO
fa = C.CDLL(os.environ["FAILALLOC_SO"])
fa.failalloc_arm.argtypes = [C.c_long, C.c_int]
fa.failalloc_class.argtypes = [C.c_int]
fa.failalloc_fired.restype = C.c_long
fa.failalloc_seen.restype = C.c_long
fa.failalloc_free_bytes.restype = C.c_longlong
C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC = 1, 2, 3
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
LEAK = 4 << 20

problems = []
report = {}


def fr(v):
    return (v % R).to_bytes(32, "big")


def load():
    return Kzg(LIB, "", precompute=0)


def walk(cls, allowed, stickies, key, call, want_ok, want_ret=C_KZG_BADARGS, noun="verdicts"):
    """call(k) -> a tuple, the return value first.  want_ok(key, want) is the driver's check of the unarmed result: None,
    or the problem in words.  want_ret is the return value of a call that got through, noun what its result holds."""
    fa.failalloc_class(cls)
    k = load()
    want = call(k)
    k.close()
    wrong = want_ok(key, want)
    if wrong:
        problems.append(wrong)
    base = fa.failalloc_free_bytes()
    for sticky in stickies:
        fired_total, seen_unarmed = 0, None
        for nth in range(0, 64):
            sys.stderr.write("[failalloc] %s: failure %d, sticky=%d\n" % (key, nth, sticky))
            k = load()
            fa.failalloc_arm(nth, sticky)
            got = call(k)
            fired, seen = fa.failalloc_fired(), fa.failalloc_seen()
            fa.failalloc_disarm()
            what = "%s %d failed (sticky=%d)" % (key, nth, sticky)
            if not fired:
                seen_unarmed = seen
                if got != want:
                    problems.append("%s: unarmed result differs" % key)
                k.close()
                break
            fired_total += 1
            if got[0] not in allowed and got != want:
                problems.append("%s -> C_KZG_RET %d" % (what, got[0]))
            if got[0] == want_ret and got != want:
                problems.append("%s -> a result, but a wrong one" % what)
            after = call(k)   # the same settings, the same call, right after the failure
            if after != want:
                problems.append("%s: call after -> C_KZG_RET %d%s" % (what, after[0], "" if after[0] != want[0] else ", wrong " + noun))
            k.close()
            d = base - fa.failalloc_free_bytes()
            if d > LEAK:
                problems.append("%s: %d bytes of device memory not returned" % (what, d))
        report.setdefault(key, {})["sticky" if sticky else "single"] = {"seen": seen_unarmed, "failures_injected": fired_total}
    fa.failalloc_class(0)
