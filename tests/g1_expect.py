"""References for the G1 sum stages (tests/test_gpu_g1_stages.py) in Python integers.

Every base is a_i * G with a chosen a_i (a_i = 0: infinity, the (0, 0) encoding), so every quantity a stage produces
is a known multiple of the generator and its expected value is one integer mod r:

    table entry (window tw, base i, e)     (e + 1) * 2^(c * tw) * a_i
    digit-vector sum                       sum_{w, i} d[w][i] * 2^(c * (w mod twin)) * lambda^[w < twin] * a_{voff + i}
    scalar-vector sum                      sum_i k_i * a_i

The integer becomes a point by ONE scalar multiplication of the CPU oracle (G1Source, memoised per scalar); whole tables
take one multiplication per base, the oracle's doublings between windows and its additions along a chain.  Byte forms (affine and XYZZ strings of the
device, table entries as tb_store_point writes them, compressed points) are made and taken apart here, in integers.

The lane walk of msm_sum_pairs (msm.hip) is replayed on discrete logarithms (replay_lane): which addition of a lane is
a load, a plain addition, a doubling or a cancellation, and the sign state `yneg` before it.  solve_events chooses bases
that force such events at chosen lanes and steps; solve_affine chooses bases that make lane sums, block partial sums or
totals equal, opposite or zero.  Both refuse (Refused) what they cannot meet and verify what they return.

tests/test_g1_expect_cpu.py checks each of these by a second route."""
import ctypes as C

from g1_points import P, R, INF, compress, sqrt_fp   # noqa: F401  (sqrt_fp: for the callers)

LAMBDA = 0xac45a4010001a40200000000ffffffff   # bls_consts32.h: FR_LAMBDA; phi(P) = [LAMBDA]P on G1
assert (LAMBDA * LAMBDA + LAMBDA + 1) % R == 0
M384 = pow(2, 384, P)
M384_INV = pow(M384, -1, P)
M392 = pow(2, 392, P)
ZERO_AFFINE = bytes(96)
ZERO_XYZZ = bytes(192)
INF48 = bytes([0xc0]) + bytes(47)


class Refused(Exception):
    """a request the solver cannot meet"""


# ---- byte forms ----

def fp_raw(v):
    """twelve little-endian words of v in the 2^384 Montgomery domain"""
    return (v * M384 % P).to_bytes(48, "little")


def fp_int(b):
    v = int.from_bytes(b, "little")
    assert v < P, "a coordinate that is not fully reduced"
    return v * M384_INV % P


def affine_raw(pt):
    return ZERO_AFFINE if pt is INF else fp_raw(pt[0]) + fp_raw(pt[1])


def affine_point(b):
    """a 96-byte affine string of the device -> (x, y) or INF; infinity is (0, 0) and nothing else"""
    if b == ZERO_AFFINE:
        return INF
    return (fp_int(b[:48]), fp_int(b[48:96]))


def table_entry_raw(pt):
    """a table entry as tb_store_point writes it: canonical, 2^392 Montgomery domain, twelve words a coordinate"""
    if pt is INF:
        return ZERO_AFFINE
    return (pt[0] * M384 * 256 % P).to_bytes(48, "little") + (pt[1] * M384 * 256 % P).to_bytes(48, "little")


def xyzz_raw(pt, z=1):
    """(x z^2, y z^3, z^2, z^3): the XYZZ string of pt with a chosen z"""
    if pt is INF:
        return ZERO_XYZZ
    zz, zzz = z * z % P, z * z * z % P
    return fp_raw(pt[0] * zz % P) + fp_raw(pt[1] * zzz % P) + fp_raw(zz) + fp_raw(zzz)


def x28_raw(pt, z=1):
    """an entry of a call-time table (X28: x, y, zz, zzz as 14 limbs of 28 bits each, a word a limb, 2^392 domain) for pt
    in the representation (x z^2, y z^3, z^2, z^3); all zero for infinity"""
    if pt is INF:
        return bytes(224)
    zz, zzz = z * z % P, z * z * z % P
    out = []
    for v in (pt[0] * zz, pt[1] * zzz, zz, zzz):
        v = v * M392 % P
        out.append(b"".join(((v >> (28 * j)) & 0xfffffff).to_bytes(4, "little") for j in range(14)))
    return b"".join(out)


def xyzz_point(b):
    """a 192-byte XYZZ string of the device as a point: infinity exactly as the product encodes it (all zero),
    zzz^2 = zz^3, and x / zz, y / zzz"""
    if b == ZERO_XYZZ:
        return INF
    x, y, zz, zzz = (fp_int(b[48 * k:48 * k + 48]) for k in range(4))
    assert zz != 0 and zzz != 0, "a finite XYZZ point with a zero denominator (infinity is the all-zero string)"
    assert zzz * zzz % P == zz * zz * zz % P, "zzz^2 != zz^3"
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


def xyzz_is(b, want):
    """the same comparison without an inversion, for outputs by the hundred thousand: b (XYZZ string) is the point
    whose affine string is `want` -- x = X zz, y = Y zzz and zzz^2 = zz^3 with zz != 0, all in the Montgomery domain
    (v_m = v 2^384: x_m 2^384 = X_m zz_m); infinity is the all-zero string and nothing else"""
    if want == ZERO_AFFINE or b == ZERO_XYZZ:
        return want == ZERO_AFFINE and b == ZERO_XYZZ
    x, y, zz, zzz = (int.from_bytes(b[48 * k:48 * k + 48], "little") for k in range(4))
    wx, wy = int.from_bytes(want[:48], "little"), int.from_bytes(want[48:], "little")
    if max(x, y, zz, zzz) >= P or zz == 0:
        return False
    return (x * M384 - wx * zz) % P == 0 and (y * M384 - wy * zzz) % P == 0 and (zzz * zzz * M384 - zz * zz % P * zz) % P == 0


def le_words(vals):
    """canonical scalars as eight little-endian words each"""
    return b"".join((v % (1 << 256)).to_bytes(32, "little") for v in vals)


# ---- scalars into points ----

class G1Source:
    """k -> k * G by the oracle's scalar multiplication, one call per distinct scalar"""

    def __init__(self, lib):
        self.lib = lib
        for fn in ("ofr_from_raw", "og1_mul", "og1_to_affine", "og1_add", "og1_batch_to_affine", "og1_dbl"):
            getattr(lib, fn).restype = None
        self.gen = (C.c_char * 144).in_dll(lib, "OG1_GENERATOR")
        self.cache = {}
        self.calls = 0

    def jac(self, k):
        """144 bytes: the oracle's Jacobian point"""
        fr, out = C.create_string_buffer(32), C.create_string_buffer(144)
        self.lib.ofr_from_raw(fr, (k % R).to_bytes(32, "little"))
        self.lib.og1_mul(out, self.gen, fr)
        self.calls += 1
        return out

    def raw(self, k):
        """96 bytes: affine, 2^384 domain, (0, 0) for k = 0 mod r"""
        k %= R
        got = self.cache.get(k)
        if got is None:
            aff = C.create_string_buffer(96)
            self.lib.og1_to_affine(aff, self.jac(k))
            got = self.cache[k] = aff.raw
        return got

    def point(self, k):
        return affine_point(self.raw(k))

    def compressed(self, k):
        return compress(self.point(k))

    def chain_raw(self, base, count):
        """(e + 1) * B for e < count as affine strings, B a Jacobian point of the oracle (not infinity): its additions"""
        jacs = C.create_string_buffer(144 * count)
        C.memmove(jacs, base, 144)
        cur = C.create_string_buffer(base.raw, 144)
        for e in range(1, count):
            self.lib.og1_add(cur, cur, base)
            C.memmove(C.byref(jacs, 144 * e), cur, 144)
        affs = C.create_string_buffer(96 * count)
        self.lib.og1_batch_to_affine(affs, jacs, C.c_size_t(count))
        return affs.raw


def twin_for(c):
    return 127 // c + 1


def table_raw(src, a, c):
    """the whole fixed-base table over the bases a_i * G: table[(tw * npoints + i) * half + e] = (e + 1) 2^(c tw) a_i G.
    One multiplication per base; the window bases by the oracle's doublings, the chains by its additions."""
    half, twin, n = 1 << (c - 1), twin_for(c), len(a)
    rows = [None] * (twin * n)
    for i, ai in enumerate(a):
        if ai % R == 0:
            for tw in range(twin):
                rows[tw * n + i] = ZERO_AFFINE * half
            continue
        base = src.jac(ai)
        for tw in range(twin):
            rows[tw * n + i] = src.chain_raw(base, half)
            for _ in range(c):
                src.lib.og1_dbl(base, base)
    out = []
    for row in rows:   # into the 2^392 domain: times 2^8
        for k in range(0, len(row), 48):
            v = int.from_bytes(row[k:k + 48], "little")
            out.append((v * 256 % P).to_bytes(48, "little"))
    return b"".join(out)


# ---- sums ----

def digit_sum(d, a, ppv, c, voff=0):
    """the discrete logarithm of the sum a digit vector d[w * ppv + i] selects"""
    twin, tot = twin_for(c), 0
    for w in range(2 * twin):
        row = sum(dv * a[voff + i] for i, dv in enumerate(d[w * ppv:(w + 1) * ppv]) if dv)
        tot += (row << (c * (w % twin))) * (LAMBDA if w < twin else 1)
    return tot % R


def scalar_sum(k, a):
    return sum(x * y for x, y in zip(k, a)) % R


def digits_value(d, c):
    """(k1, k2) of the nwin digits of one scalar: windows 0 .. twin - 1 are k2 (the phi half)"""
    twin = twin_for(c)
    assert len(d) == 2 * twin
    return (sum(d[twin + w] << (c * w) for w in range(twin)), sum(d[w] << (c * w) for w in range(twin)))


# ---- the lane walk ----

class Shape:
    """one vector of a fixed-base sum as the accumulate kernels cut it: pairs q = w * ppv + i, workgroup `block` owns
    [block * ppb, (block + 1) * ppb), lane l of it the pairs block * ppb + l + m * stride"""

    def __init__(self, npoints, ppv, stride, ppb, c, voff=0, lanes=None):
        self.npoints, self.ppv, self.stride, self.c, self.voff = npoints, ppv, stride, c, voff
        self.twin = twin_for(c)
        self.pairs = 2 * self.twin * ppv
        self.phi_pairs = self.twin * ppv
        self.ppb = min(ppb, self.pairs) if ppb else self.pairs
        self.bpv = (self.pairs + self.ppb - 1) // self.ppb
        self.lanes = lanes if lanes else stride
        assert voff + ppv <= npoints

    def lane_pairs(self, block, lane):
        q0 = block * self.ppb
        return range(q0 + lane, min(q0 + self.ppb, self.pairs), self.stride)

    def pair(self, q):
        """(base index, 2^(c * tw)) of pair q"""
        w = q // self.ppv
        return self.voff + q - w * self.ppv, 1 << (self.c * (w % self.twin))


def replay_lane(shape, d, a, block, lane):
    """(discrete log of the lane's sum, [(step, kind, yneg before, first addition after phi)]) -- msm_sum_pairs with
    xyzz28_madd_alt on discrete logarithms; kind is load / add / double / cancel; a table entry at infinity is skipped"""
    acc, inf, yneg, step, events = 0, True, False, 0, []
    pairs = shape.lane_pairs(block, lane)
    phi_pending = len(pairs) > 0 and pairs[0] < shape.phi_pairs
    just_phi = False
    for q in pairs:
        if phi_pending and q >= shape.phi_pairs:
            if not inf:
                acc, just_phi = acc * LAMBDA % R, True
            phi_pending = False
        if d[q] == 0:
            continue
        i, coef = shape.pair(q)
        e = d[q] * coef * a[i] % R
        if e == 0:
            continue
        before = yneg
        if inf:
            acc, inf, yneg, kind = e, False, True, "load"
        elif acc == e:
            acc, yneg, kind = 2 * e % R, False, "double"
        elif (acc + e) % R == 0:
            acc, inf, yneg, kind = 0, True, False, "cancel"
        else:
            acc, yneg, kind = (acc + e) % R, not yneg, "add"
        events.append((step, kind, before, just_phi))
        just_phi = False
        step += 1
    if phi_pending and not inf:
        acc = acc * LAMBDA % R
    return acc, events


def lane_sum(shape, d, a, block, lane):
    """the same discrete log as a linear form of the bases (no walk)"""
    tot = 0
    for q in shape.lane_pairs(block, lane):
        if d[q]:
            i, coef = shape.pair(q)
            tot += d[q] * coef * a[i] * (LAMBDA if q < shape.phi_pairs else 1)
    return tot % R


def block_sum(shape, d, a, block):
    return sum(lane_sum(shape, d, a, block, l) for l in range(shape.lanes)) % R


def predict(shape, d, a):
    """{"lanes": [block][lane], "blocks": [block], "total", "events": {(block, lane): [...]}} by the replayed walk"""
    lanes, events = [], {}
    for b in range(shape.bpv):
        row = []
        for l in range(shape.lanes):
            v, ev = replay_lane(shape, d, a, b, l)
            row.append(v)
            if any(k in ("double", "cancel") for _, k, _, _ in ev):
                events[(b, l)] = ev
        lanes.append(row)
    blocks = [sum(row) % R for row in lanes]
    return {"lanes": lanes, "blocks": blocks, "total": sum(blocks) % R, "events": events}


# ---- the solvers ----

KINDS = ("double", "cancel", "cancel_go_on", "after_phi")


def solve_events(shape, d, wanted, a, rnd):
    """bases with every wanted event satisfied.  wanted: dicts {block, lane, step, kind, yneg (optional)}; kind
    `double` / `cancel`: the lane's addition number `step` (counting its non-zero digits from 0) meets acc == entry /
    acc == -entry; `cancel_go_on`: a cancellation that at least one more addition follows; `after_phi`: a doubling at
    the first addition after the accumulator went through phi (step is not used).  yneg: the sign state before the
    event.  a: the bases, None where the solver is free.  Solves a_i' = +-acc / (d' 2^(c tw')) lane by lane; a base
    an earlier lane's history read is not touched again.  Returns (a, {(block, lane): events of the replay})."""
    a = list(a)
    locked = {i for i, v in enumerate(a) if v is not None}

    def fill(i):
        if a[i] is None:
            a[i] = rnd.randrange(1, R)
        locked.add(i)
        return a[i]

    for ev in wanted:
        if ev["kind"] not in KINDS:
            raise Refused("unknown kind %r" % (ev["kind"],))
        acc, inf, yneg, step, hit, more = 0, True, False, 0, False, False
        pairs = shape.lane_pairs(ev["block"], ev["lane"])
        phi_pending = len(pairs) > 0 and pairs[0] < shape.phi_pairs
        just_phi = False
        for q in pairs:
            if phi_pending and q >= shape.phi_pairs:
                if not inf:
                    acc, just_phi = acc * LAMBDA % R, True
                phi_pending = False
            if d[q] == 0:
                continue
            i, coef = shape.pair(q)
            if hit:   # cancel_go_on: the addition that follows
                fill(i)
                more = a[i] != 0
                if more:
                    break
                continue
            here = just_phi if ev["kind"] == "after_phi" else step == ev["step"]
            if here:
                if inf:
                    raise Refused("lane %r: the accumulator is at infinity where the event is wanted" % (ev,))
                if i in locked:
                    raise Refused("lane %r: base %d of the event is already fixed" % (ev, i))
                if ev.get("yneg") is not None and ev["yneg"] != yneg:
                    raise Refused("lane %r: yneg is %r before the event" % (ev, yneg))
                sign = -1 if ev["kind"] in ("cancel", "cancel_go_on") else 1
                a[i] = sign * acc * pow(d[q] * coef, -1, R) % R
                locked.add(i)
                hit = True
                if ev["kind"] != "cancel_go_on":
                    break
                continue
            e = d[q] * coef * fill(i) % R
            if e == 0:
                continue
            if inf:
                acc, inf, yneg = e, False, True
            elif acc == e:
                acc, yneg = 2 * e % R, False
            elif (acc + e) % R == 0:
                acc, inf, yneg = 0, True, False
            else:
                acc, yneg = (acc + e) % R, not yneg
            just_phi = False
            step += 1
        if not hit:
            raise Refused("lane %r has no such addition" % (ev,))
        if ev["kind"] == "cancel_go_on" and not more:
            raise Refused("lane %r: nothing follows the cancellation" % (ev,))
    for i in range(len(a)):
        if a[i] is None:
            a[i] = rnd.randrange(1, R)
    seen = {}
    for ev in wanted:   # nothing is dropped silently: the replay must show every event
        _, got = replay_lane(shape, d, a, ev["block"], ev["lane"])
        seen[(ev["block"], ev["lane"])] = got
        kind = "cancel" if ev["kind"].startswith("cancel") else "double"
        if ev["kind"] == "after_phi":
            ok = any(k == kind and phi for _, k, _, phi in got)
        else:
            ok = any(s == ev["step"] and k == kind and (ev.get("yneg") is None or y == ev["yneg"]) for s, k, y, _ in got)
        if ok and ev["kind"] == "cancel_go_on":
            at = next(s for s, k, _, _ in got if k == "cancel" and s == ev["step"])
            ok = any(s > at for s, _, _, _ in got)
        if not ok:
            raise Refused("lane %r: the replay does not show the event" % (ev,))
    return a, seen


def solve_affine(constraints, a, free):
    """set a[free[j]] so that every constraint(a) == 0 mod r; each constraint is affine in the bases (differences of
    lane_sum / block_sum / digit_sum values).  As many constraints as free bases; a singular system is refused."""
    n = len(free)
    if n != len(constraints):
        raise Refused("%d constraints for %d free bases" % (len(constraints), n))
    a = list(a)
    for j in free:
        a[j] = 0
    f0 = [c(a) % R for c in constraints]
    m = [[0] * (n + 1) for _ in range(n)]
    for col, j in enumerate(free):
        a[j] = 1
        for row, c in enumerate(constraints):
            m[row][col] = (c(a) - f0[row]) % R
        a[j] = 0
    for row in range(n):
        m[row][n] = -f0[row] % R
    for col in range(n):
        piv = next((r_ for r_ in range(col, n) if m[r_][col]), None)
        if piv is None:
            raise Refused("the constraints do not determine base %d" % free[col])
        m[col], m[piv] = m[piv], m[col]
        inv = pow(m[col][col], -1, R)
        m[col] = [v * inv % R for v in m[col]]
        for r_ in range(n):
            if r_ != col and m[r_][col]:
                f = m[r_][col]
                m[r_] = [(v - f * w) % R for v, w in zip(m[r_], m[col])]
    for col, j in enumerate(free):
        a[j] = m[col][n]
    if any(c(a) % R for c in constraints):
        raise Refused("the solution does not satisfy the constraints")
    return a
