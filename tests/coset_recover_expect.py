"""The model of ckzg_hip_recover_cosets_and_kzg_proofs_rows in Python integers: which rows are valid, where the plan puts
every held coset, which sets are distinct, what the device gets as missing lists, how a coset's product is sliced over
`parts` lanes, and the factors themselves -- the vanishing polynomial of the missing cosets, constant over a coset.

Coset size l = 2^e; m = 8192 >> e cosets a row.  Position p = l c + k of a row has the natural index brp13(p), whose low
13 - e bits are b(c) = brp_{13-e}(c).  With w_m = w^l:
    Z over the domain, coset c          = prod over missing j of (      w_m^b(c) - w_m^b(j))
    Z over the shifted coset, coset c   = prod over missing j of (7^l * w_m^b(c) - w_m^b(j))
"""
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
W = pow(7, (R - 1) // 8192, R)          # roots_of_unity[1] of the 8192-point domain
EXT = 8192
NONE = 0xffffffff
FILL_WAVES = 1024                       # one wave per SIMD: 256 CUs x 4
MIN_CHAIN = 32


def brp(v, bits):
    return int(format(v, "0%db" % bits)[::-1], 2) if bits else 0


def cosets(e):
    return EXT >> e


def root_index(j, e):
    """index into roots_of_unity of w_m^b(j)"""
    return brp(j, 13 - e) << e


_ROOTS = []


def roots():
    """w^i, i <= 8192"""
    if not _ROOTS:
        v = 1
        for _ in range(EXT + 1):
            _ROOTS.append(v)
            v = v * W % R
    return _ROOTS


def row_valid(idx, e):
    m = cosets(e)
    return m // 2 <= len(idx) <= m and all(0 <= c < m for c in idx) and all(a < b for a, b in zip(idx, idx[1:]))


def plan(rows, e, chunk_rows):
    """rows: lists of coset indices.  Returns (per_row, chunks): per_row[r] = None for an invalid row, else (chunk, device
    row, set id); chunks[c] = dict(rows=[caller rows], sets=[tuples of held cosets, in order of first appearance],
    runs=[(caller row, device row, rows, cosets)], missing=[per set the root indices of its missing cosets])."""
    m = cosets(e)
    per_row, chunks, prev = [], [], False
    for r, idx in enumerate(rows):
        if not row_valid(list(idx), e):
            per_row.append(None)
            prev = False
            continue
        if not chunks or len(chunks[-1]["rows"]) == chunk_rows:
            chunks.append(dict(rows=[], sets=[], runs=[], missing=[]))
            prev = False
        ch = chunks[-1]
        key = tuple(idx)
        if key not in ch["sets"]:
            ch["sets"].append(key)
            held = set(key)
            ch["missing"].append([root_index(j, e) for j in range(m) if j not in held])
        dev = len(ch["rows"])
        ch["rows"].append(r)
        per_row.append((len(chunks) - 1, dev, ch["sets"].index(key)))
        if prev:
            a, b, n, k = ch["runs"][-1]
            ch["runs"][-1] = (a, b, n + 1, k + len(idx))
        else:
            ch["runs"].append((r, dev, 1, len(idx)))
        prev = True
    return per_row, chunks


def parts(sets, e):
    """lanes per coset of the factor launch: doubled while the launch has fewer waves than SIMDs and the slices of the
    longest list (m / 2 factors) would keep MIN_CHAIN steps"""
    m, p = cosets(e), 1
    while sets * m * p // 64 < FILL_WAVES and (m // 2) // (2 * p) >= MIN_CHAIN:
        p *= 2
    return p


def all_parts(e):
    """every value the picker can return at this e"""
    out, p = [1], 1
    while (cosets(e) // 2) // (2 * p) >= MIN_CHAIN and cosets(e) * p // 64 < FILL_WAVES:
        p *= 2
        out.append(p)
    return out


def slices(count, nparts):
    """[lo, hi) of the missing list for each part: contiguous, every slice ceil(count / parts) steps, the tail empty"""
    step = -(-count // nparts)
    return [(min(q * step, count), min((q + 1) * step, count)) for q in range(nparts)]


def factors(missing_cosets, which, e):
    """(Z over the domain, 1 / Z over the shifted coset) for the cosets `which`; missing_cosets: coset indices"""
    rt, l = roots(), 1 << e
    seven_l = pow(7, l, R)
    rj = [rt[root_index(j, e)] for j in missing_cosets]
    zd, zi = [], []
    for c in which:
        x = rt[root_index(c, e)]
        xs = seven_l * x % R
        pd = pc = 1
        for v in rj:
            pd = pd * (x - v) % R
            pc = pc * (xs - v) % R
        zd.append(pd)
        zi.append(pow(pc, R - 2, R))
    return zd, zi


def closed_form(first_half_missing, c, e):
    """(Z over the domain, Z over the shifted coset) at coset c when the first (c < m / 2: b even) or the second half of
    the cosets is missing: short(y) = y^(m/2) -+ 1, and (w_m^b)^(m/2) = (-1)^b, (7^l)^(m/2) = 7^4096."""
    sign = -1 if brp(c, 13 - e) & 1 else 1
    k = -1 if first_half_missing else 1
    return (sign + k) % R, (pow(7, 4096, R) * sign + k) % R


def limbs(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def le32(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)
