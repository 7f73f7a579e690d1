// host_shim.cpp -- exports the header-only host/device arithmetic through a C ABI so the CPU
// test-suite (tests/test_host_arith.py) can compare it limb for limb with the oracle.  Built with
// plain g++ (no GPU needed); it is a test aid for the product's own headers, not part of
// libckzg_hip.so.
#include <vector>
#include "host_pairing.hpp"
using namespace ckzg;
using namespace ckzg::host;

extern "C" {
void hs_fp_mul(Fp *r, const Fp *a, const Fp *b) { *r = mul(*a, *b); }
void hs_fp_add(Fp *r, const Fp *a, const Fp *b) { *r = add(*a, *b); }
void hs_fp_sub(Fp *r, const Fp *a, const Fp *b) { *r = sub(*a, *b); }
void hs_fp_inv(Fp *r, const Fp *a) { *r = fp_inv(*a); }
void hs_fr_mul(Fr *r, const Fr *a, const Fr *b) { *r = mul(*a, *b); }
void hs_fr_add(Fr *r, const Fr *a, const Fr *b) { *r = add(*a, *b); }
void hs_fr_sub(Fr *r, const Fr *a, const Fr *b) { *r = sub(*a, *b); }
void hs_fr_inv(Fr *r, const Fr *a) { *r = fr_inv(*a); }
// G1: all in/out as Jacobian (blst_p1 layout)
void hs_g1_add_jac(G1Jac *r, const G1Jac *a, const G1Jac *b) { *r = jac_add(*a, *b); }
void hs_g1_dbl_jac(G1Jac *r, const G1Jac *a) { *r = jac_dbl(*a); }
void hs_g1_add_xyzz(G1Jac *r, const G1Jac *a, const G1Jac *b) {
    *r = jac_from_xyzz(xyzz_add(xyzz_from_jac(*a), xyzz_from_jac(*b)));
}
void hs_g1_madd_xyzz(G1Jac *r, const G1Jac *a, const G1Affine *b) {
    G1XYZZ acc = xyzz_from_jac(*a);
    xyzz_madd(acc, *b);
    *r = jac_from_xyzz(acc);
}
void hs_g1_madd_jac(G1Jac *r, const G1Jac *a, const G1Affine *b) { *r = jac_madd(*a, *b); }
void hs_g1_dbl_xyzz(G1Jac *r, const G1Jac *a) { *r = jac_from_xyzz(xyzz_dbl(xyzz_from_jac(*a))); }
void hs_g1_mul(G1Jac *r, const G1Jac *a, const uint32_t *k, int nbits) { *r = jac_mul(*a, k, nbits); }
void hs_g1_compress(uint8_t *out, const G1Jac *a) { g1_compress_affine(out, jac_to_affine(*a)); }
int hs_g1_uncompress(G1Affine *out, const uint8_t *in) { return g1_uncompress(*out, in); }
void hs_g1_xyzz_to_affine(G1Affine *out, const G1Jac *a) { *out = xyzz_to_affine(xyzz_from_jac(*a)); }
int hs_g2_uncompress(G2Affine *out, const uint8_t *in) { return g2_uncompress(*out, in); }
int hs_pairings_verify(const G1Jac *a1, const G2Jac *a2, const G1Jac *b1, const G2Jac *b2) {
    return pairings_verify(*a1, *a2, *b1, *b2) ? 1 : 0;
}
void hs_g2_mul(G2Jac *r, const G2Jac *a, const uint32_t *k, int nbits) { *r = g2_mul(*a, k, nbits); }
void hs_g2_generator(G2Jac *r) { *r = g2_generator(); }
void hs_g1_generator(G1Jac *r) { *r = g1_generator(); }
// portable compression loop only (the dispatching Sha256 picks SHA-NI when the CPU has it)
void hs_sha256_portable(uint8_t *out, const uint8_t *msg, size_t len) {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    size_t nb = len / 64;
    for (size_t i = 0; i < nb; i++) sha256_block(h, msg + 64 * i);
    uint8_t tail[128] = {0};
    size_t rem = len - 64 * nb;
    memcpy(tail, msg + 64 * nb, rem);
    tail[rem] = 0x80;
    size_t tl = rem < 56 ? 64 : 128;
    uint64_t bits = (uint64_t)len * 8;
    for (int i = 0; i < 8; i++) tail[tl - 1 - i] = (uint8_t)(bits >> (8 * i));
    for (size_t i = 0; i < tl / 64; i++) sha256_block(h, tail + 64 * i);
    for (int i = 0; i < 8; i++) {
        out[4 * i] = (uint8_t)(h[i] >> 24); out[4 * i + 1] = (uint8_t)(h[i] >> 16);
        out[4 * i + 2] = (uint8_t)(h[i] >> 8); out[4 * i + 3] = (uint8_t)h[i];
    }
}
int hs_cpu_has_sha_ni() {
#ifdef CKZG_HAVE_SHANI
    return cpu_has_sha_ni() ? 1 : 0;
#else
    return 0;
#endif
}
void hs_sha256(uint8_t *out, const uint8_t *msg, size_t len) {
    Sha256 s;
    // feed in awkward pieces to exercise the buffering
    size_t a = len / 3;
    s.update(msg, a);
    s.update(msg + a, len - a);
    s.finish(out);
}
}

// ---- 28-bit-limb device arithmetic (fp28.hpp / g1_28.hpp), exercised on the host ----
#include "g1_28.hpp"
#include "fr_inv.hpp"
extern "C" {
// r = a*b in the 2^384 domain, computed through the 2^392-domain multiplier
void hs_fp28_mul(Fp *r, const Fp *a, const Fp *b) { *r = f28_to_fp(mul(f28_from_fp(*a), f28_from_fp(*b))); }
void hs_fp28_roundtrip(Fp *r, const Fp *a) { *r = f28_to_fp(f28_from_fp(*a)); }
void hs_fp28_sub(Fp *r, const Fp *a, const Fp *b) { *r = f28_to_fp(sub(f28_from_fp(*a), f28_from_fp(*b))); }
void hs_fp28_addchain(Fp *r, const Fp *a, const Fp *b) {
    auto x = f28_from_fp(*a), y = f28_from_fp(*b);
    *r = f28_to_fp(norm(sub(add(add(x, y), x), add(y, y))));  // 2a - b
}
// r = (-a)*b through cneg_reduced (a must be fully reduced, as table coordinates are)
void hs_fp28_cneg_mul(Fp *r, const Fp *a, const Fp *b, int negate) {
    Fp k;
    for (int i = 0; i < 12; i++) k.l[i] = FP_MONT_2POW8[i];
    Fp t = mul(*a, k);  // a in the 2^392 domain, fully reduced, packed
    *r = f28_to_fp(mul(cneg_reduced(f28_unpack<1>(t.l), negate != 0), f28_from_fp(*b)));
}
// table entries are stored as the 32-bit-domain product with 2^8, packed; emulate that path
static F28<1, 1> table_coord(const Fp &v) {
    Fp k;
    for (int i = 0; i < 12; i++) k.l[i] = FP_MONT_2POW8[i];
    Fp t = mul(v, k);
    return f28_unpack<1>(t.l);
}
// acc (Jacobian, may be infinity) += +-pt (affine) through xyzz28_madd
void hs_g1_madd28(G1Jac *r, const G1Jac *acc_in, const G1Affine *pt, int negate) {
    XYZZ28 acc;
    bool inf = acc_in->is_inf();
    if (!inf) {
        G1XYZZ a = xyzz_from_jac(*acc_in);
        acc.x = widen<1, 10>(f28_from_fp(a.x));
        acc.y = widen<1, 6>(f28_from_fp(a.y));
        acc.zz = f28_from_fp(a.zz);
        acc.zzz = f28_from_fp(a.zzz);
    }
    xyzz28_madd(acc, inf, table_coord(pt->x), cneg_reduced(table_coord(pt->y), negate != 0));
    *r = jac_from_xyzz(xyzz28_to_xyzz(acc, inf));
}
void hs_g1_add28(G1Jac *r, const G1Jac *a, const G1Jac *b) {
    bool ai, bi;
    XYZZ28 x = xyzz28_from_xyzz(xyzz_from_jac(*a), ai), y = xyzz28_from_xyzz(xyzz_from_jac(*b), bi);
    xyzz28_add(x, ai, y, bi);
    *r = jac_from_affine(xyzz28_to_affine(x, ai));
}
void hs_g1_mul28(G1Jac *r, const G1Jac *a, const uint32_t *k) {
    bool ai, oi;
    XYZZ28 x = xyzz28_from_xyzz(xyzz_from_jac(*a), ai), o;
    xyzz28_mul_w4(o, oi, x, ai, k);
    *r = jac_from_affine(xyzz28_to_affine(o, oi));
}
// subgroup test and square root of the device validation path; returns 1 in / 0 out / 2 not on curve
int hs_g1_in_subgroup28(const G1Affine *pt) {
    auto x = f28_from_fp(pt->x), y = f28_from_fp(pt->y);
    F28<1, 2> yy;
    if (!g1_28_solve_y(yy, x)) return 2;
    if (!f28_equal(yy, y) && !is_zero(mul(add(yy, y), f28_one()))) return 3;  // sqrt must be +-y
    return g1_28_in_subgroup(x, y) ? 1 : 0;
}
void hs_glv_split(uint32_t *k1k2, const uint32_t *k) { glv_split(k, k1k2, k1k2 + 4); }
void hs_g1_mul28_glv(G1Jac *r, const G1Jac *a, const uint32_t *k) {
    uint32_t glv[8];
    glv_split(k, glv, glv + 4);
    bool ai, oi;
    XYZZ28 x = xyzz28_from_xyzz(xyzz_from_jac(*a), ai), o;
    xyzz28_mul_glv_w4(o, oi, x, ai, glv);
    *r = jac_from_affine(xyzz28_to_affine(o, oi));
}
void hs_wnaf4_128(int8_t *out, const uint32_t *k) { wnaf4_128(out, k); }
void hs_g1_mul28_glv_naf(G1Jac *r, const G1Jac *a, const uint32_t *k) {
    uint32_t glv[8];
    glv_split(k, glv, glv + 4);
    int8_t naf[2 * GLV_NAF_LEN];
    wnaf4_128(naf, glv);
    wnaf4_128(naf + GLV_NAF_LEN, glv + 4);
    bool ai, oi;
    XYZZ28 x = xyzz28_from_xyzz(xyzz_from_jac(*a), ai), o;
    xyzz28_mul_glv_naf(o, oi, x, ai, naf, naf + GLV_NAF_LEN);
    *r = jac_from_affine(xyzz28_to_affine(o, oi));
}
// The co-Z table of the NAF ladder and its mixed addition, step by step: r[m] = tbl[m] brought home (m = 0..3:
// P, 3P, 5P, 7P); then with acc on the table's curve: r[4] = inf + P, r[5] = P + P (the equal-points branch),
// r[6] = 2P + 3P (generic), r[7] = 5P + (-5P) (must be infinity), r[8] = 2P + phi-entry of 7P.
void hs_je28_cases(G1Jac *r, const G1Jac *a) {
    bool ai;
    XYZZ28 x = xyzz28_from_xyzz(xyzz_from_jac(*a), ai);
    EAT28 tbl[4];
    F28<1, 2> zc;
    eat28_build(tbl, zc, x);
    auto home = [&](const JE28 &acc, bool inf) {
        if (inf) return jac_from_affine(xyzz28_to_affine(x, true));
        JAC28 j;
        j.x = widen<1, 34>(acc.x);
        j.y = widen<1, 34>(acc.y);
        j.z = widen<2, 4>(mul(acc.z, zc));
        return jac_from_affine(xyzz28_to_affine(jac28_to_xyzz(j), false));
    };
    for (int m = 0; m < 4; m++) {
        JE28 acc;
        bool inf = true;
        je28_madd(acc, inf, tbl[m].x, tbl[m].y, false);
        r[m] = home(acc, inf);
    }
    JE28 acc;
    bool inf = true;
    je28_madd(acc, inf, tbl[0].x, tbl[0].y, false);
    r[4] = home(acc, inf);
    je28_madd(acc, inf, tbl[0].x, tbl[0].y, false);
    r[5] = home(acc, inf);
    JE28 two = acc;
    je28_madd(acc, inf, tbl[1].x, tbl[1].y, false);
    r[6] = home(acc, inf);
    je28_madd(acc, inf, tbl[2].x, tbl[2].y, true);
    r[7] = home(acc, inf);
    acc = two;
    inf = false;
    je28_madd(acc, inf, tbl[3].bx, tbl[3].y, false);
    r[8] = home(acc, inf);
}
// a + (+-b) and 2a through the Jacobian 28-bit-limb formulas (b must be finite)
void hs_g1_jac28_add(G1Jac *r, const G1Jac *a, const G1Jac *b, int negate_b) {
    bool ai, bi;
    XYZZ28 xa = xyzz28_from_xyzz(xyzz_from_jac(*a), ai), xb = xyzz28_from_xyzz(xyzz_from_jac(*b), bi);
    JAC28 ja;
    if (!ai) ja = jac28_from_xyzz(xa);
    JACT28 tb = jac28_table_entry(jac28_from_xyzz(xb));
    if (negate_b) tb = jact28_neg(tb);
    jac28_add(ja, ai, tb);
    XYZZ28 o;
    if (!ai) o = jac28_to_xyzz(ja);
    *r = jac_from_affine(xyzz28_to_affine(o, ai));
}
void hs_g1_jac28_dbl_chain(G1Jac *r, const G1Jac *a, int n) {
    bool ai;
    XYZZ28 xa = xyzz28_from_xyzz(xyzz_from_jac(*a), ai);
    JAC28 ja = jac28_from_xyzz(xa);
    for (int i = 0; i < n; i++) jac28_dbl(ja);
    *r = jac_from_affine(xyzz28_to_affine(jac28_to_xyzz(ja), false));
}
void hs_g1_neg28(G1Jac *r, const G1Jac *a) {
    bool ai;
    XYZZ28 x = xyzz28_from_xyzz(xyzz_from_jac(*a), ai);
    *r = jac_from_affine(xyzz28_to_affine(xyzz28_neg(x), ai));
}
// r = a*b + c*d with one reduction, operands lazily reduced the way xyzz28_madd_alt feeds them:
// (a + a) as <2,4>, (b - c) as <4,18>
void hs_fp28_mul_add2(Fp *r, const Fp *a, const Fp *b, const Fp *c, const Fp *d) {
    auto fa = f28_from_fp(*a), fb = f28_from_fp(*b), fc = f28_from_fp(*c), fd = f28_from_fp(*d);
    auto a2 = add(fa, fa);                              // <2,4>
    auto bc = sub(fb, widen<1, 10>(fc));                // <4,18>
    *r = f28_to_fp(mul_add2(a2, bc, widen<1, 6>(fc), fd));  // 2a(b-c) + c*d
}
// chain through xyzz28_madd_alt (sign-alternating accumulator): signs[i] != 0 subtracts pts[i]
void hs_g1_madd28_alt_chain(G1Jac *r, const G1Affine *pts, const uint8_t *signs, int n) {
    XYZZ28 acc;
    bool inf = true, yneg = false;
    for (int i = 0; i < n; i++)
        xyzz28_madd_alt(acc, inf, yneg, table_coord(pts[i].x), table_coord(pts[i].y), signs[i] != 0);
    xyzz28_fix_sign(acc, inf, yneg);
    *r = jac_from_xyzz(xyzz28_to_xyzz(acc, inf));
}
// many additions in a row, to exercise the value-bound bookkeeping over a long chain
void hs_g1_madd28_chain(G1Jac *r, const G1Affine *pts, int n) {
    XYZZ28 acc;
    bool inf = true;
    for (int i = 0; i < n; i++) xyzz28_madd(acc, inf, table_coord(pts[i].x), cneg_reduced(table_coord(pts[i].y), (i & 1) != 0));
    *r = jac_from_xyzz(xyzz28_to_xyzz(acc, inf));
}
}

// Consistency of the fast Fp12 routines with the generic product, on pseudo-random inputs derived
// from `seed`: bit 0 complex squaring, bit 1 sparse line product, bit 2 cyclotomic squaring (on an
// element of the cyclotomic subgroup), bit 3 cyclotomic squaring must DIFFER on a generic element
// (guards against a test that cannot fail).  Returns 0 when everything agrees.
extern "C" int hs_g1_in_subgroup_host(const G1Affine *a) { return g1_in_subgroup_host(*a) ? 1 : 0; }
extern "C" void hs_g1_mul_glv_host(G1Jac *r, const G1Jac *p, const uint32_t *k) { *r = g1_mul_glv_host(*p, k); }

extern "C" void hs_fr_inv_safegcd(Fr *r, const Fr *a) { *r = fr_inv_safegcd(*a); }
extern "C" void hs_fr_inv_fermat(Fr *r, const Fr *a) { *r = fr_inv(*a); }

// timing helpers (tools only): n pairing-product checks with prepared G2 arguments / n Fp products
extern "C" int hs_bench_pairing(const G1Jac *a1, const G2Jac *q1, const G1Jac *a2, const G2Jac *q2, int n) {
    G2Prepared p1, p2;
    g2_prepare(p1, g2_to_affine(*q1));
    g2_prepare(p2, g2_to_affine(*q2));
    G1Affine x1 = jac_to_affine(*a1), x2 = jac_to_affine(*a2);
    int ok = 0;
    for (int i = 0; i < n; i++) ok += pairing_product_is_one(x1, p1, x2, p2) ? 1 : 0;
    return ok;
}
// n final exponentiations of a fixed Miller-loop value (timing only)
extern "C" int hs_bench_final_exp(const G1Jac *a1, const G2Jac *q1, int n) {
    Fp12 f = miller_loop(g2_to_affine(*q1), jac_to_affine(*a1));
    int ones = 0;
    for (int i = 0; i < n; i++) ones += is_one(final_exp(f)) ? 1 : 0;
    return ones;
}
extern "C" void hs_bench_fp_mul(Fp *r, const Fp *a, const Fp *b, int n) {
    Fp x = *a;
    for (int i = 0; i < n; i++) x = mul(x, *b);
    *r = x;
}

extern "C" int hs_fp12_selftest(uint32_t seed) {
    auto rnd_fp = [&](uint32_t i) {
        uint8_t in[8], d[64];
        memcpy(in, &seed, 4);
        memcpy(in + 4, &i, 4);
        Sha256 a;
        a.update(in, 8);
        a.finish(d);
        Sha256 b;
        b.update(d, 32);
        b.finish(d + 32);
        uint32_t raw[12];
        memcpy(raw, d, 48);
        raw[11] &= 0x0fffffffu;  // < p
        return from_raw<FpParams>(raw);
    };
    uint32_t ctr = 0;
    auto rnd_fp2 = [&]() { Fp2 r = {rnd_fp(ctr), rnd_fp(ctr + 1)}; ctr += 2; return r; };
    auto rnd_fp12 = [&]() {
        Fp12 f;
        f.c0 = {rnd_fp2(), rnd_fp2(), rnd_fp2()};
        f.c1 = {rnd_fp2(), rnd_fp2(), rnd_fp2()};
        return f;
    };
    auto same = [](const Fp12 &a, const Fp12 &b) { return std::memcmp(&a, &b, sizeof a) == 0; };
    int bad = 0;
    Fp12 f = rnd_fp12();
    if (!same(sqr(f), mul(f, f))) bad |= 1;
    {
        Fp2 lam = rnd_fp2(), c = rnd_fp2();
        G1Affine p = {rnd_fp(ctr), rnd_fp(ctr + 1)};
        ctr += 2;
        Fp12 l;
        std::memset(&l, 0, sizeof l);
        l.c0.c0 = c;
        l.c0.c1 = neg(mul_fp(lam, p.x));
        l.c1.c1.c0 = p.y;
        if (!same(mul_by_prepared_line(f, lam, c, p), mul(f, l))) bad |= 2;
    }
    Fp12 a = mul(conj(f), inv(f));
    a = mul(frobenius<2>(a), a);  // in the cyclotomic subgroup
    if (!same(cyclotomic_sqr(a), mul(a, a))) bad |= 4;
    if (same(cyclotomic_sqr(f), mul(f, f))) bad |= 8;
    // bit 4: the lazily reduced Fp2 product and square against the schoolbook formulas on Fp
    for (int rep = 0; rep < 8; rep++) {
        Fp2 x = rnd_fp2(), y = rnd_fp2();
        if (rep == 0) y = x;
        if (rep == 1) { x.c0 = Fp::zero(); y.c1 = Fp::zero(); }
        if (rep == 2) { x.c0 = neg(Fp::one()); x.c1 = neg(Fp::one()); y = x; }  // p - 1 in both slots
        Fp2 want = {sub(mul(x.c0, y.c0), mul(x.c1, y.c1)), add(mul(x.c0, y.c1), mul(x.c1, y.c0))};
        Fp2 got = mul(x, y);
        if (!(got == want)) bad |= 16;
        Fp2 sq = sqr(x), sqw = {sub(mul(x.c0, x.c0), mul(x.c1, x.c1)), dbl(mul(x.c0, x.c1))};
        if (!(sq == sqw)) bad |= 16;
    }
    return bad;
}

// [k]G1 from the generator table against the generic ladder; returns 1 when they agree
extern "C" int hs_g1_gen_mul_check(const uint32_t *k) {
    G1Jac a = g1_gen_mul(k), b = g1_mul_glv_host(g1_generator(), k);
    G1Affine x = jac_to_affine(a), y = jac_to_affine(b);
    return std::memcmp(&x, &y, sizeof x) == 0 ? 1 : 0;
}
// the product check with the second pair's Miller loop run separately (what verify_blob_kzg_proof does underneath
// the GPU's evaluation) against the fused loop: returns verdict | (agreement << 1)
extern "C" int hs_pairing_split(const G1Jac *a1, const G2Jac *q1, const G1Jac *a2, const G2Jac *q2) {
    G2Prepared p1, p2;
    g2_prepare(p1, g2_to_affine(*q1));
    g2_prepare(p2, g2_to_affine(*q2));
    const G1Affine x1 = jac_to_affine(*a1), x2 = jac_to_affine(*a2);
    const Fp12 early = miller_product_prepared(x2, p2, G1Affine::inf(), p2);
    const Fp12 late = miller_product_prepared(x1, p1, G1Affine::inf(), p1);
    const bool split = is_one(final_exp(mul(late, early)));
    const bool fused = pairing_product_is_one(x1, p1, x2, p2);
    return (split ? 1 : 0) | ((split == fused) ? 2 : 0);
}

extern "C" int hs_pairing_prepared(const G1Jac *a1, const G2Jac *q1, const G1Jac *a2, const G2Jac *q2) {
    G2Prepared p1, p2;
    g2_prepare(p1, g2_to_affine(*q1));
    g2_prepare(p2, g2_to_affine(*q2));
    return pairing_product_is_one(jac_to_affine(*a1), p1, jac_to_affine(*a2), p2) ? 1 : 0;
}

extern "C" {
void hs_fp28_sqr(Fp *r, const Fp *a) { *r = f28_to_fp(sqr(f28_from_fp(*a))); }
// square of a lazily reduced operand (limbs up to 4 units, value up to 18p): (a - b)^2
void hs_fp28_sqr_lazy(Fp *r, const Fp *a, const Fp *b) {
    auto d = sub(f28_from_fp(*a), widen<1, 10>(f28_from_fp(*b)));  // <4,18>
    *r = f28_to_fp(sqr(d));
}
void hs_fp28_inv(Fp *r, const Fp *a) { *r = f28_to_fp(f28_inv_fermat(f28_from_fp(*a))); }
}

extern "C" void hs_fp28_inv_safegcd(Fp *r, const Fp *a) { *r = f28_to_fp(f28_inv_safegcd(f28_from_fp(*a))); }

// balanced GLV split + signed window recoding of the fixed-base MSM kernels (g1_28.hpp)
extern "C" void hs_glv_split_signed(const uint32_t *k, uint32_t *m1, int *neg1, uint32_t *m2, int *neg2) {
    bool n1, n2;
    glv_split_signed(k, m1, n1, m2, n2);
    *neg1 = n1;
    *neg2 = n2;
}
extern "C" void hs_recode_signed_128(int16_t *dst, const uint32_t *m, int neg, int wbits, int nwh) {
    recode_signed_128(dst, 1, m, neg != 0, wbits, nwh);
}

// The fixed-base MSM kernels' algorithm (msm.hip: k_msm_accumulate / k_msm_small) replayed on the host
// with the very same inline functions: GLV digits, table entries (mag * 2^(wbits*tw) * P_i, computed here
// on demand instead of read from HBM), sign-alternating mixed additions, phi applied once per lane when it
// crosses from the k2 half into the k1 half, lane partials folded with xyzz28_add.
extern "C" void hs_msm_glv_emulate(G1Jac *r, const G1Affine *pts, const uint32_t *scalars, int n, int wbits,
                                   int lanes) {
    const int twin = 127 / wbits + 1, nwin = 2 * twin;
    std::vector<int16_t> dg((size_t)nwin * n);
    for (int i = 0; i < n; i++) {
        uint32_t m1[4], m2[4];
        bool n1, n2;
        glv_split_signed(scalars + 8 * i, m1, n1, m2, n2);
        recode_signed_128(dg.data() + i, n, m2, n2, wbits, twin);
        recode_signed_128(dg.data() + (size_t)twin * n + i, n, m1, n1, wbits, twin);
    }
    const uint32_t pairs = (uint32_t)nwin * n, phi_pairs = pairs / 2;
    XYZZ28 total;
    bool tinf = true;
    for (int l = 0; l < lanes; l++) {
        XYZZ28 acc;
        bool inf = true, yneg = false, phi_pending = (uint32_t)l < phi_pairs;
        for (uint32_t q = l; q < pairs; q += lanes) {
            if (phi_pending && q >= phi_pairs) {
                if (!inf) acc.x = widen<1, 10>(mul(acc.x, f28_const<1, 1>(FP28_BETA_LAMBDA)));
                phi_pending = false;
            }
            int d = dg[q];
            if (d == 0) continue;
            uint32_t w = q / n, i = q - w * n, tw = w >= (uint32_t)twin ? w - twin : w;
            uint32_t mag = (uint32_t)(d < 0 ? -d : d);
            G1Jac e = jac_from_affine(pts[i]);
            for (uint32_t k = 0; k < tw * (uint32_t)wbits; k++) e = jac_dbl(e);
            G1Jac m = G1Jac::inf();
            for (int b = 31; b >= 0; b--) {
                m = jac_dbl(m);
                if ((mag >> b) & 1u) m = jac_add(m, e);
            }
            if (m.is_inf()) continue;  // a table entry at infinity is skipped by the kernels too
            G1Affine a = jac_to_affine(m);
            xyzz28_madd_alt(acc, inf, yneg, table_coord(a.x), table_coord(a.y), d < 0);
        }
        if (phi_pending && !inf) acc.x = widen<1, 10>(mul(acc.x, f28_const<1, 1>(FP28_BETA_LAMBDA)));
        xyzz28_fix_sign(acc, inf, yneg);
        xyzz28_add(total, tinf, acc, inf);
    }
    *r = jac_from_affine(xyzz28_to_affine(total, tinf));
}

// ---- Fr on 29-bit limbs (fr29.hpp) and the barycentric evaluation built on it, replayed thread by thread ----
#include "fr29.hpp"
extern "C" void hs_fr29_mul(Fr *r, const Fr *a, const Fr *b) { *r = fr29_to_fr(fr29_mul(fr29_from_fr(*a), fr29_from_fr(*b))); }
// the radix travels with the operand: (a 2^256) (b 2^261) / 2^261 is the library's form of a b
extern "C" void hs_fr29_mul_mixed(Fr *r, const Fr *a, const Fr *b) {
    fr29_unpack(r->l, fr29_canonical<0>(fr29_mul(fr29_pack(a->l), fr29_from_fr(*b))));
}
extern "C" void hs_fr29_roundtrip(Fr *r, const Fr *a) { *r = fr29_to_fr(fr29_from_fr(*a)); }
extern "C" void hs_fr29_inv(Fr *r, const Fr *a) { *r = fr29_to_fr(fr29_inv(fr29_from_fr(*a))); }
extern "C" void hs_fr29_sub(Fr *r, const Fr *a, const Fr *b) {
    *r = fr29_to_fr(fr29_sub_canonical(fr29_from_fr(*a), fr29_from_fr(*b)));
}
// sum of n values through the lazy additions and the closing ladder (n <= 32)
extern "C" void hs_fr29_sum(Fr *r, const Fr *a, int n) {
    Fr29 s;
    for (int i = 0; i < 9; i++) s.l[i] = 0;
    for (int k = 0; k < n; k++) {
        Fr29 t = fr29_pack(a[k].l);
        for (int j = 0; j < 9; j++) s.l[j] += t.l[j];
        if ((k & 3) == 3) fr29_carry(s);
    }
    fr29_carry(s);
    *r = ev29::to_fr_radix256(s);
}
// One blob through the kernel's algorithm (verify.hip: k_eval_barycentric): 512 threads of 8 terms, one inversion
// per lane of the first wave for the eight waves' products.  Returns the index of the domain point equal to z (y =
// p[hit]) or -1; di_out (may be null): 4096 x 8 words, 1/(z - w_i) in the 2^261 radix, canonical.
extern "C" int hs_fr29_eval(Fr *y, uint32_t *di_out, const Fr *poly, const Fr *z, const Fr *brp_roots) {
    constexpr int T = 64 * ev29::WAVES, NB = 4096;
    static_assert(T * ev29::PER == NB, "geometry");
    std::vector<Fr29> roots29(NB), pre((size_t)T * ev29::PER), acc(T), parked(T), inv(T);
    for (int i = 0; i < NB; i++) roots29[i] = fr29_from_fr(brp_roots[i]);
    const Fr29 z29 = fr29_from_fr(*z);
    int hit = -1;
    for (int t = 0; t < T; t++) {
        int h = ev29::forward(&pre[(size_t)t * ev29::PER], acc[t], z29, roots29.data(), t, T);
        if (h >= 0) hit = h;
    }
    if (hit >= 0) {
        *y = poly[hit];
        return hit;
    }
    for (int l = 0; l < 64; l++)
        ev29::invert_across([&](int w) { return acc[l + 64 * w]; }, [&](int w, const Fr29 &v) { parked[l + 64 * w] = v; },
                            [&](int w) { return parked[l + 64 * w]; }, [&](int w, const Fr29 &v) { inv[l + 64 * w] = v; },
                            [](const Fr29 &v) { return fr29_inv(v); });
    Fr sum = Fr::zero();
    for (int t = 0; t < T; t++)
        sum = add(sum, ev29::to_fr_radix256(ev29::backward(&pre[(size_t)t * ev29::PER], inv[t], z29, roots29.data(), poly, t, T, di_out)));
    *y = ev29::scale(sum, ev29::vanishing_over_n(z29));
    return -1;
}

// The quotient of the opening at the domain point z = brp_roots[m] through k_quotient_in_domain's algorithm (512
// threads of 8 terms, ev29::forward<true>, one inversion per lane of the first wave, ev29::quotient_in_domain, q_m from
// the roots table's 1/w).  q_out: 4096 x 8 words, canonical integers.
extern "C" void hs_fr29_quotient_in_domain(uint32_t *q_out, const Fr *poly, int m, const Fr *brp_roots) {
    constexpr int T = 64 * ev29::WAVES, NB = 4096;
    std::vector<Fr29> roots29(NB + NB / 2), pre((size_t)T * ev29::PER), acc(T), parked(T), inv(T);
    for (int i = 0; i < NB; i++) roots29[i] = fr29_from_fr(brp_roots[i]);
    for (int j = 0; j < NB / 2; j++) roots29[NB + j] = fr29_canonical<0>(fr29_inv(roots29[2 * j]));
    const Fr29 z = roots29[m];
    for (int t = 0; t < T; t++) (void)ev29::forward<true>(&pre[(size_t)t * ev29::PER], acc[t], z, roots29.data(), t, T);
    for (int l = 0; l < 64; l++)
        ev29::invert_across([&](int w) { return acc[l + 64 * w]; }, [&](int w, const Fr29 &v) { parked[l + 64 * w] = v; },
                            [&](int w) { return parked[l + 64 * w]; }, [&](int w, const Fr29 &v) { inv[l + 64 * w] = v; },
                            [](const Fr29 &v) { return fr29_inv(v); });
    Fr sum = Fr::zero();
    for (int t = 0; t < T; t++)
        sum = add(sum, ev29::to_fr_radix256(ev29::quotient_in_domain(
                           &pre[(size_t)t * ev29::PER], inv[t], z, roots29.data(), poly, poly[m], m, t, T,
                           [&](int i, const uint32_t *raw) { memcpy(q_out + (size_t)i * 8, raw, 32); })));
    const Fr s = (m & 1) ? sum : sub(Fr::zero(), sum);
    fr29_unpack(q_out + (size_t)m * 8, fr29_canonical<0>(fr29_mul(fr29_pack(s.l), roots29[NB + (m >> 1)])));
}

// One blob through k_eval_tree<LOG_PER>'s algorithm: 4096 >> LOG_PER threads each fold 2^LOG_PER leaves, six levels
// of lane exchanges inside a wave (both lanes of a pair compute the parent), the waves' values by thread 0.
// bytes != nullptr: the leaves come from the blob's bytes (k_eval_tree's BYTES form); *bad |= 1 for an element >= r.
template <int LOG_PER>
static void eval_tree_emulate(Fr *y, const Fr *poly, const Fr *z, const Fr *brp_roots, const uint8_t *bytes = nullptr,
                              uint32_t *bad = nullptr) {
    constexpr int NB = 4096, T = NB >> LOG_PER, W = T / 64;
    std::vector<Fr29> tab(NB / 2), v(T), nv(T);
    for (int m = 0; m < NB / 2; m++) tab[m] = fr29_inv(fr29_from_fr(brp_roots[2 * m]));
    for (auto &t : tab) t = fr29_canonical<0>(t);
    Fr29 zp[12];
    zp[0] = fr29_from_fr(*z);
    for (int l = 1; l < 12; l++) zp[l] = fr29_mul(zp[l - 1], zp[l - 1]);
    uint32_t any_bad = 0;
    auto leaf = [&](int i) {
        if (!bytes) return fr29_pack(poly[i].l);
        uint32_t s[8];
        for (int k = 0; k < 8; k++) {
            const uint8_t *q = bytes + 32 * i + 4 * (7 - k);
            s[k] = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3];
        }
        return ev29::tree_leaf_from_words(s, any_bad);
    };
    for (int t = 0; t < T; t++)
        v[t] = ev29::tree_canonical<LOG_PER>(ev29::tree_node<LOG_PER>(leaf, tab.data(), zp, t << LOG_PER));
    if (bad) *bad |= any_bad;
    for (int k = 0; k < 6; k++) {
        for (int t = 0; t < T; t++) {
            const bool odd = (t >> k) & 1;
            const Fr29 &mine = v[t], &other = v[t ^ (1 << k)];
            nv[t] = fr29_canonical<1>(ev29::tree_combine<0>(odd ? other : mine, odd ? mine : other,
                                                            fr29_mul(zp[LOG_PER + k], tab[t >> (k + 1)])));
        }
        v.swap(nv);
    }
    Fr29 a[W > 1 ? W : 1];
    for (int w = 0; w < W; w++) a[w] = v[64 * w];
    int lvl = LOG_PER + 6;
    for (int n = W; n > 1; n >>= 1, lvl++)
        for (int m = 0; m < n / 2; m++)
            a[m] = fr29_canonical<1>(ev29::tree_combine<0>(a[2 * m], a[2 * m + 1], fr29_mul(zp[lvl], tab[m])));
    *y = bytes ? ev29::tree_finish_from_integers(a[0]) : ev29::tree_finish(a[0]);
}
extern "C" void hs_fr29_eval_tree_bytes(Fr *y, uint32_t *bad, const uint8_t *blob, const Fr *z, const Fr *brp_roots, int log_per) {
    if (log_per == 6) eval_tree_emulate<6>(y, nullptr, z, brp_roots, blob, bad);
    else eval_tree_emulate<4>(y, nullptr, z, brp_roots, blob, bad);
}
extern "C" void hs_fr29_eval_tree(Fr *y, const Fr *poly, const Fr *z, const Fr *brp_roots, int log_per) {
    if (log_per == 6) eval_tree_emulate<6>(y, poly, z, brp_roots);
    else eval_tree_emulate<4>(y, poly, z, brp_roots);
}

// The host's pairing (host_pairing.hpp on tower.hpp, here with the lazily reduced 64-bit Fp2 forms) for
// tests/test_point_pairing_host.py, which holds the 32-bit-body build of the same tower and the device's Miller product
// (libfield32_shim.so) to it byte for byte.  Fp12 values are 576-byte Montgomery limb arrays.
extern "C" {
void hs_host_final_exp(Fp12 *r, const Fp12 *f) { *r = final_exp(*f); }
void hs_host_fp12_inv(Fp12 *r, const Fp12 *f) { *r = inv(*f); }
void hs_host_fp12_mul(Fp12 *r, const Fp12 *a, const Fp12 *b) { *r = mul(*a, *b); }
// Miller product with G2 arguments prepared by g2_prepare
void hs_host_miller(Fp12 *r, const G1Jac *a1, const G2Jac *q1, const G1Jac *a2, const G2Jac *q2) {
    G2Prepared p1, p2;
    g2_prepare(p1, g2_to_affine(*q1));
    g2_prepare(p2, g2_to_affine(*q2));
    *r = miller_product_prepared(jac_to_affine(*a1), p1, jac_to_affine(*a2), p2);
}
}

// ---- The cell check by groups at coset size 2^e (ckzg_hip_verify_coset_kzg_proof_batch_groups; the cell call by groups
// at e = 6: hs_cell_groups_replay below) -- the kernels of coset_groups.hip (k_coset_group_rlc_scalars, k_group_commit_weights, k_coset_group_aggregate,
// k_coset_group_interp with its butterfly stages, k_coset_group_interp_sum) replayed slot by slot over the index maps
// the product builds (coset_groups_plan.hpp), so that the maps can be checked without a GPU
// (tests/test_coset_groups_cpu.py).  Field elements cross as canonical little-endian limbs: evals [N][l], r [G], roots
// w^i [8193].  Out: info = (total, quad, pairs, rows, parts of the aggregation, parts of the per-group sum), term_src
// [total], part_off [2 G + 1] and the jobs' scalars sc [total][8].  Returns the number of terms, -1 if it exceeds
// cap_terms, -2 for e out of range. ----
#include "coset_groups_plan.hpp"
extern "C" long hs_coset_groups_replay(uint32_t *sc, uint32_t *term_src, uint32_t *part_off, uint32_t *info, size_t cap_terms,
                                       const uint64_t *start, size_t G, const uint32_t *item_commit, size_t num_commits,
                                       const uint64_t *coset_indices, const uint32_t *evals_raw, const uint32_t *r_raw,
                                       const uint32_t *roots_raw, int e, size_t quad_max_terms) {
    if (e < 0 || e > COSET_MAX_LOG) return -2;
    CosetGroupsPlan p;
    build_coset_groups_plan(p, start, G, item_commit, num_commits, coset_indices, e, quad_max_terms);
    if (p.total > cap_terms) return -1;
    const size_t N = p.N, l = (size_t)1 << e;
    info[0] = (uint32_t)p.total;
    info[1] = p.quad ? 1 : 0;
    info[2] = (uint32_t)p.P;
    info[3] = (uint32_t)p.R;
    info[4] = coset_groups_agg_parts(N, p.R);
    info[5] = coset_groups_sum_parts(p.R, G);
    for (size_t t = 0; t < p.total; t++) term_src[t] = p.term_src[t];
    for (size_t j = 0; j <= 2 * G; j++) part_off[j] = p.part_off[j];
    for (size_t t = 0; t < p.total * 8; t++) sc[t] = 0;
    auto fr_at = [](const uint32_t *raw, size_t i) { return from_raw<FrParams>(raw + i * 8); };
    const uint32_t *gd = p.gd.data();
    // k_coset_group_rlc_scalars
    std::vector<Fr> rp(N);
    for (size_t i = 0; i < N; i++) {
        const uint32_t g = p.item_grp[i], off = (uint32_t)i - gd[g];
        Fr base = fr_at(r_raw, g), pw = Fr::one();
        for (uint32_t x = off; x; x >>= 1) {
            if (x & 1u) pw = mul(pw, base);
            base = mul(base, base);
        }
        rp[i] = pw;
        const size_t ta = (size_t)gd[G + 1 + g] + gd[2 * G + 1 + g] + off, tb = (size_t)gd[3 * G + 1 + g] + off;
        to_raw<FrParams>(sc + ta * 8, mul(pw, fr_at(roots_raw, coset_verify_shift_root(p.item_col[i], e))));
        to_raw<FrParams>(sc + tb * 8, pw);
    }
    // k_group_commit_weights
    for (size_t j = 0; j < p.P; j++) {
        Fr acc = Fr::zero();
        for (uint32_t q = p.pair_start[j]; q < p.pair_start[j + 1]; q++) acc = add(acc, rp[p.pair_members[q]]);
        to_raw<FrParams>(sc + (size_t)p.pair_term[j] * 8, acc);
    }
    // k_coset_group_aggregate, then k_coset_group_interp over the R l slots
    std::vector<Fr> rows(p.R * l), next(p.R * l);
    for (size_t slot = 0; slot < p.R * l; slot++) {
        const size_t t = slot >> e, j = slot & (l - 1);
        Fr acc = Fr::zero();
        for (uint32_t q = p.row_start[t]; q < p.row_start[t + 1]; q++) {
            const uint32_t i = p.row_order[q];
            acc = add(acc, mul(fr_at(evals_raw, ((size_t)i << e) + j), rp[i]));
        }
        rows[slot] = acc;
    }
    for (int s = 1; s <= e; s++) {
        const uint32_t half = 1u << (s - 1);
        for (size_t slot = 0; slot < p.R * l; slot++) {
            const uint32_t k = (uint32_t)(slot & (l - 1));
            const Fr v = rows[slot], other = rows[slot ^ half], tw = fr_at(roots_raw, coset_verify_twiddle_root(k, s));
            next[slot] = (k & half) ? sub(other, mul(v, tw)) : add(v, mul(other, tw));
        }
        rows.swap(next);
    }
    const uint32_t l_raw[8] = {(uint32_t)l, 0, 0, 0, 0, 0, 0, 0};
    const Fr inv_l = fr_inv(from_raw<FrParams>(l_raw));
    for (size_t slot = 0; slot < p.R * l; slot++) {
        const uint32_t k = (uint32_t)(slot & (l - 1));
        rows[slot] = mul(mul(rows[slot], inv_l), fr_at(roots_raw, coset_verify_unshift_root(p.row_col[slot >> e], e, k)));
    }
    // k_coset_group_interp_sum
    for (size_t g = 0; g < G; g++) {
        const uint32_t n = gd[g + 1] - gd[g];
        if (!n) continue;
        for (uint32_t k = 0; k < l; k++) {
            Fr acc = Fr::zero();
            for (uint32_t t = p.grp_rows[g]; t < p.grp_rows[g + 1]; t++) acc = add(acc, rows[((size_t)t << e) + k]);
            to_raw<FrParams>(sc + ((size_t)gd[G + 1 + g] + gd[2 * G + 1 + g] + n + k) * 8, neg(acc));
        }
    }
    return (long)p.total;
}

// ckzg_hip_verify_cell_kzg_proof_batch_groups: the same at e = 6 -- cells [N][64], info = (total, quad, pairs, rows)
// (tests/test_cell_groups_cpu.py)
extern "C" long hs_cell_groups_replay(uint32_t *sc, uint32_t *term_src, uint32_t *part_off, uint32_t *info, size_t cap_terms,
                                      const uint64_t *start, size_t G, const uint32_t *cell_commit, size_t num_commits,
                                      const uint64_t *cell_indices, const uint32_t *cells_raw, const uint32_t *r_raw,
                                      const uint32_t *roots_raw, size_t quad_max_terms) {
    uint32_t info6[6];
    const long total = hs_coset_groups_replay(sc, term_src, part_off, info6, cap_terms, start, G, cell_commit, num_commits,
                                              cell_indices, cells_raw, r_raw, roots_raw, 6, quad_max_terms);
    if (total >= 0) memcpy(info, info6, 4 * sizeof(uint32_t));
    return total;
}

// ---- ckzg_hip_verify_blob_kzg_proof_batch_groups: the segmented scalar arithmetic of verify.hip
// (k_blob_group_scalars, k_blob_group_ysum) replayed element by element over the index maps the product builds
// (blob_groups_plan.hpp), so that the maps can be checked without a GPU (tests/test_blob_groups_cpu.py).  Field
// elements cross as canonical little-endian limbs: z [N], y [N], r [G].  Out: the plan's sizes in info (total, quad),
// term_src [total], part_off [2 G + 1] and the jobs' scalars sc [total][8].  Returns the number of terms, or -1 if it
// exceeds cap_terms. ----
#include "blob_groups_plan.hpp"
extern "C" long hs_blob_groups_replay(uint32_t *sc, uint32_t *term_src, uint32_t *part_off, uint32_t *info, size_t cap_terms,
                                      const uint64_t *start, size_t G, const uint32_t *z_raw, const uint32_t *y_raw,
                                      const uint32_t *r_raw, size_t quad_max_terms) {
    BlobGroupsPlan p;
    build_blob_groups_plan(p, start, G, quad_max_terms);
    if (p.total > cap_terms) return -1;
    const size_t N = p.N;
    info[0] = (uint32_t)p.total;
    info[1] = p.quad ? 1 : 0;
    for (size_t t = 0; t < p.total; t++) term_src[t] = p.term_src[t];
    for (size_t j = 0; j <= 2 * G; j++) part_off[j] = p.part_off[j];
    for (size_t t = 0; t < p.total * 8; t++) sc[t] = 0;
    auto fr_at = [](const uint32_t *raw, size_t i) { return from_raw<FrParams>(raw + i * 8); };
    const uint32_t *gd = p.gd.data();
    // k_blob_group_scalars
    std::vector<Fr> ry(N);
    for (size_t i = 0; i < N; i++) {
        const uint32_t g = p.blob_grp[i], a = gd[g], off = (uint32_t)i - a, ng = gd[g + 1] - a;
        Fr base = fr_at(r_raw, g), pw = Fr::one();
        for (uint32_t e = off; e; e >>= 1) {
            if (e & 1u) pw = mul(pw, base);
            base = mul(base, base);
        }
        ry[i] = mul(pw, fr_at(y_raw, i));
        const size_t tc = (size_t)gd[G + 1 + g] + off, tp = tc + ng, tb = (size_t)gd[2 * G + 1 + g] + off;
        to_raw<FrParams>(sc + tc * 8, pw);
        to_raw<FrParams>(sc + tp * 8, mul(pw, fr_at(z_raw, i)));
        to_raw<FrParams>(sc + tb * 8, pw);
    }
    // k_blob_group_ysum: lane l of the group's wave takes blobs a + l, a + l + 64, ...; then the butterfly
    for (size_t g = 0; g < G; g++) {
        const uint32_t a = gd[g], b = gd[g + 1];
        if (a == b) continue;
        Fr lane[64];
        for (uint32_t l = 0; l < 64; l++) {
            lane[l] = Fr::zero();
            for (uint32_t i = a + l; i < b; i += 64) lane[l] = add(lane[l], ry[i]);
        }
        if (b - a > 1) {
            for (uint32_t m = 32; m >= 1; m >>= 1) {
                Fr nxt[64];
                for (uint32_t l = 0; l < 64; l++) nxt[l] = add(lane[l], lane[l ^ m]);
                for (uint32_t l = 0; l < 64; l++) lane[l] = nxt[l];
            }
        }
        to_raw<FrParams>(sc + ((size_t)gd[G + 1 + g] + 2 * (size_t)(b - a)) * 8, neg(lane[0]));
    }
    return (long)p.total;
}

// ---- recovery by rows at coset size 2^e: the index maps the product builds (coset_recover_plan.hpp) laid out per
// caller row and per caller coset, and the per-coset factor arithmetic of k_coset_recover_factors
// (coset_recover_factors.hpp: the very function the kernel calls) replayed for one set, so that both can be checked
// without a GPU (tests/test_coset_recover_cpu.py; at e = 6, in the cell call's terms, tests/test_recover_rows_cpu.py).
// Plan: per caller row valid / chunk / device row / set id inside the chunk / the set's mask as the plan stores it
// (row_mask [num_rows][m / 32]); per caller coset its position in the chunk's device input (through the copy runs) and
// the scatter target stored for that position, 0xffffffff for the cosets of invalid rows; chunk_info [chunks][info] =
// rows, cosets, sets, all_full and, where info is 5, the entries of the missing lists.  Returns the number of chunks, -1
// for a malformed row_start or e > 6, -2 beyond cap_chunks. ----
#include "coset_recover_plan.hpp"
#include "coset_recover_factors.hpp"
static long coset_recover_plan_out(uint8_t *valid, uint32_t *row_chunk, uint32_t *row_dev, uint32_t *row_set,
                                   uint32_t *row_mask, uint32_t *coset_pos, uint32_t *coset_dst, uint32_t *chunk_info,
                                   size_t info, size_t cap_chunks, const uint64_t *coset_indices,
                                   const uint64_t *row_start, uint64_t num_rows, int e, size_t chunk_rows) {
    if (e < 0 || e > COSET_RECOVER_MAX_LOG || !slice_starts_ok(row_start, num_rows)) return -1;
    const uint32_t W = coset_recover_mask_words(e);
    CosetRecoverPlan p;
    build_coset_recover_plan(p, coset_indices, row_start, num_rows, e, chunk_rows);
    if (p.chunks.size() > cap_chunks) return -2;
    for (uint64_t r = 0; r < num_rows; r++) {
        valid[r] = p.valid[(size_t)r];
        row_chunk[r] = row_dev[r] = row_set[r] = 0xffffffffu;
        for (uint32_t w = 0; w < W; w++) row_mask[W * r + w] = 0;
    }
    for (uint64_t i = 0; i < row_start[num_rows]; i++) coset_pos[i] = coset_dst[i] = 0xffffffffu;
    for (size_t c = 0; c < p.chunks.size(); c++) {
        const CosetRecoverChunk &ch = p.chunks[c];
        chunk_info[info * c] = (uint32_t)ch.rows();
        chunk_info[info * c + 1] = (uint32_t)ch.cosets();
        chunk_info[info * c + 2] = (uint32_t)ch.sets();
        chunk_info[info * c + 3] = ch.all_full ? 1 : 0;
        if (info > 4) chunk_info[info * c + 4] = (uint32_t)ch.miss.size();
        for (size_t d = 0; d < ch.rows(); d++) {
            const uint64_t r = ch.row_caller[d];
            row_chunk[r] = (uint32_t)c;
            row_dev[r] = (uint32_t)d;
            row_set[r] = ch.row_set[d];
            for (uint32_t w = 0; w < W; w++) row_mask[W * r + w] = ch.set_mask[(size_t)W * ch.row_set[d] + w];
        }
        for (const CosetRecoverRun &run : ch.runs) {
            for (uint32_t j = 0; j < run.cosets; j++) {
                coset_pos[run.src_coset + j] = run.dev_coset + j;
                coset_dst[run.src_coset + j] = ch.coset_dst[run.dev_coset + j];
            }
        }
    }
    return (long)p.chunks.size();
}
extern "C" long hs_coset_recover_plan(uint8_t *valid, uint32_t *row_chunk, uint32_t *row_dev, uint32_t *row_set,
                                      uint32_t *row_mask, uint32_t *coset_pos, uint32_t *coset_dst, uint32_t *chunk_info,
                                      size_t cap_chunks, const uint64_t *coset_indices, const uint64_t *row_start,
                                      uint64_t num_rows, int e, size_t chunk_rows) {
    return coset_recover_plan_out(valid, row_chunk, row_dev, row_set, row_mask, coset_pos, coset_dst, chunk_info, 5,
                                  cap_chunks, coset_indices, row_start, num_rows, e, chunk_rows);
}
// the cell call's plan: e = 6, so row_mask [num_rows][4], and chunk_info [chunks][4]
extern "C" long hs_recover_rows_plan(uint8_t *valid, uint32_t *row_chunk, uint32_t *row_dev, uint32_t *row_set,
                                     uint32_t *row_mask, uint32_t *cell_pos, uint32_t *cell_dst, uint32_t *chunk_info,
                                     size_t cap_chunks, const uint64_t *cell_indices, const uint64_t *row_start,
                                     uint64_t num_rows, size_t chunk_rows) {
    return coset_recover_plan_out(valid, row_chunk, row_dev, row_set, row_mask, cell_pos, cell_dst, chunk_info, 4,
                                  cap_chunks, cell_indices, row_start, num_rows, 6, chunk_rows);
}

// the missing list of set `set` of chunk `chunk` of the same plan, as the device gets it: the number of entries (up to
// `cap` of them copied), -1 as above or for a chunk or set the plan does not have; runs[cap_runs][4] = caller row, device
// row, rows, cosets of the chunk's copy runs, *num_runs how many it has
extern "C" long hs_coset_recover_plan_set(uint32_t *miss, size_t cap, uint64_t *runs, size_t cap_runs, uint32_t *num_runs,
                                          const uint64_t *coset_indices, const uint64_t *row_start, uint64_t num_rows, int e,
                                          size_t chunk_rows, size_t chunk, size_t set) {
    if (e < 0 || e > COSET_RECOVER_MAX_LOG || !slice_starts_ok(row_start, num_rows)) return -1;
    CosetRecoverPlan p;
    build_coset_recover_plan(p, coset_indices, row_start, num_rows, e, chunk_rows);
    if (chunk >= p.chunks.size() || set >= p.chunks[chunk].sets()) return -1;
    const CosetRecoverChunk &ch = p.chunks[chunk];
    const uint32_t a = ch.miss_start[set], b = ch.miss_start[set + 1];
    for (uint32_t i = a; i < b && i - a < cap; i++) miss[i - a] = ch.miss[i];
    *num_runs = (uint32_t)ch.runs.size();
    for (size_t i = 0; i < ch.runs.size() && i < cap_runs; i++) {
        runs[4 * i] = ch.runs[i].caller_row;
        runs[4 * i + 1] = ch.runs[i].dev_row;
        runs[4 * i + 2] = ch.runs[i].rows;
        runs[4 * i + 3] = ch.runs[i].cosets;
    }
    return (long)(b - a);
}

extern "C" uint32_t hs_coset_recover_parts(uint64_t sets, int e) { return coset_recover_parts((size_t)sets, e); }
extern "C" uint32_t hs_coset_recover_block(int e, uint32_t parts) { return coset_recover_block(e, parts); }
extern "C" uint32_t hs_coset_recover_slice_len(uint32_t count, uint32_t parts) { return coset_recover_slice_len(count, parts); }
extern "C" uint32_t hs_coset_recover_slice_valid(uint32_t count, uint32_t parts, uint32_t q) {
    return coset_recover_slice_valid(count, parts, q);
}

// The factor kernel replayed for the cosets cosets[ncosets] of ONE set, with `parts` lanes a coset: the slices of
// coset_recover_plan.hpp, the chain of coset_recover_factors.hpp per (coset, part), the kernel's fold over the parts.
// Field elements cross as canonical little-endian limbs: roots w^i [8193], seven_l = 7^l; miss[count] as the plan makes
// it.  out: Z over the domain and 1 / Z over the shifted coset, [ncosets] each.
extern "C" void hs_coset_recover_factors(uint32_t *z_domain, uint32_t *z_coset_inv, const uint32_t *miss, uint32_t count,
                                         const uint32_t *cosets, uint32_t ncosets, int e, uint32_t parts,
                                         const uint32_t *roots_raw, const uint32_t *seven_l_raw) {
    std::vector<Fr> roots(8193);
    for (size_t i = 0; i < roots.size(); i++) roots[i] = from_raw<FrParams>(roots_raw + 8 * i);
    const Fr seven_l = from_raw<FrParams>(seven_l_raw);
    const uint32_t len = coset_recover_slice_len(count, parts);
    std::vector<Fr> pd(parts), pc(parts);
    for (uint32_t i = 0; i < ncosets; i++) {
        const Fr xd = roots[coset_recover_brp(cosets[i], e) << e], xc = mul(seven_l, xd);
        for (uint32_t q = 0; q < parts; q++) {
            pd[q] = pc[q] = Fr::one();
            coset_recover_chain(pd[q], pc[q], xd, xc, len, coset_recover_slice_valid(count, parts, q), [&](uint32_t t) {
                const uint32_t at = q * len + t;
                return roots[at < count ? miss[at] : 0u];
            });
        }
        for (uint32_t s2 = parts >> 1; s2 >= 1; s2 >>= 1) {
            for (uint32_t q = 0; q < s2; q++) {
                pd[q] = mul(pd[q], pd[q + s2]);
                pc[q] = mul(pc[q], pc[q + s2]);
            }
        }
        to_raw<FrParams>(z_domain + 8 * i, pd[0]);
        to_raw<FrParams>(z_coset_inv + 8 * i, fr_inv_safegcd(pc[0]));
    }
}

// The cell call's factors: all 128 cells of the set `mask` (4 words, bit c of word c / 32 = cell c is held) at e = 6,
// with the parts the product takes for a chunk of one set; seven64 = 7^64.  out: [128] each.
extern "C" void hs_recover_set_factors(uint32_t *z_domain, uint32_t *z_coset_inv, const uint32_t *mask,
                                       const uint32_t *roots_raw, const uint32_t *seven64_raw) {
    std::vector<uint32_t> miss, cells(128);
    coset_recover_missing(miss, mask, 6);
    for (uint32_t c = 0; c < 128; c++) cells[c] = c;
    hs_coset_recover_factors(z_domain, z_coset_inv, miss.data(), (uint32_t)miss.size(), cells.data(), 128, 6,
                             coset_recover_parts(1, 6), roots_raw, seven64_raw);
}

// ---- raw-limb entry points: the F28 operations at the bound combinations the group law instantiates
// (f28_test_ops.hpp), limbs taken as they come so that a test can pass lazily reduced operands at the edge of
// their bounds.  n items of 14 words per operand; returns 0, or 1 for an operation number past the list. ----
#include "f28_test_ops.hpp"
extern "C" const char *hs_f28_ops() { return f28test::desc(); }
extern "C" int hs_f28_run(int op, uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                          int n) {
    for (int i = 0; i < n; i++)
        if (!f28test::run(op, out + 14 * i, a + 14 * i, b + 14 * i, c + 14 * i, d + 14 * i)) return 1;
    return 0;
}

// ---- the plain NAF of the pipelined G1-FFT ladders (naf2.hpp): n scalars of 4 words -> n * NAF2_LEN digits ----
#include "naf2.hpp"
extern "C" void hs_naf2_128(int8_t *out, const uint32_t *k, int n) {
    for (int i = 0; i < n; i++) quad::naf2_128(out + quad::NAF2_LEN * i, k + 4 * i);
}

// ---- raw-word entry points: Mont<Fp> / Mont<Fr>, Fr29, the safegcd inversions and the pairing tower
// (field_test_ops.hpp).  n items; operand k of item i lies at k + width * i, the shared operands (line tables) at k.
// Returns 0, or 1 for an operation number past the list. ----
#include "field_test_ops.hpp"
extern "C" const char *hs_field_ops() { return fieldtest::desc(); }
extern "C" int hs_field_run(int op, uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                            int n) {
    return fieldtest::run_items(op, out, a, b, c, d, n) ? 0 : 1;
}
// the line table of a G2 point as k_pairing_check reads it: lam[68] then c[68] (host_pairing.hpp: g2_prepare)
extern "C" void hs_g2_line_table(uint32_t *out, const G2Jac *q) {
    G2Prepared p;
    g2_prepare(p, g2_to_affine(*q));
    memcpy(out, p.lam, sizeof p.lam);
    memcpy(out + sizeof p.lam / 4, p.c, sizeof p.c);
}

// ---- ckzg_hip_verify_kzg_proof_batch_locate / ckzg_hip_verify_blob_kzg_proof_batch_locate: the host half
// (locate_plan.hpp), checked without a GPU (tests/test_locate_cpu.py). ----
#include "locate_plan.hpp"
// The bisection over the predicate "no bad item in the range" (an invalid item is inert, as on the device, whatever its
// bad byte says).  max_checks < 0: no hand-over.  Out: ok[n], open_out[n] = 1 for the items of the ranges left open at
// hand-over, stats[0] = checks, stats[1] = open ranges.
extern "C" void hs_locate_bisect(uint8_t *ok, uint64_t *stats, uint8_t *open_out, const uint8_t *bad, const uint8_t *invalid,
                                 uint64_t n, int64_t max_checks) {
    std::vector<uint8_t> okb(n ? n : 1);
    auto range_ok = [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++)
            if (bad[i] && !invalid[i]) return false;
        return true;
    };
    auto serial = [](size_t m, auto &&fn) {
        for (size_t i = 0; i < m; i++) fn(i);
    };
    const LocateOutcome res = locate_bisect(reinterpret_cast<bool *>(okb.data()), invalid, (size_t)n,
                                            max_checks < 0 ? UINT64_MAX : (uint64_t)max_checks, range_ok, serial);
    for (uint64_t i = 0; i < n; i++) {
        ok[i] = okb[i];
        open_out[i] = 0;
    }
    for (const LocateRange &r : res.open)
        for (size_t i = r.a; i < r.b; i++) open_out[i] = 1;
    stats[0] = res.checks;
    stats[1] = res.open.size();
}

// The whole second half of the point form in host arithmetic: validation, P1_i = C_i - [y_i]G + [z_i]proof_i, the
// challenge r (locate_point_digest), A_i = [r^i]P1_i and B_i = [r^i]proof_i, their prefix sums, and the bisection over
// the real predicate e(PA[b] - PA[a], [1]_2) * e(-(PB[b] - PB[a]), [tau]_2) == 1.  tau_g2: [tau]_2 (g2_values_monomial[1]).
// Out: ok[n], status[n] (1 = invalid item), stats[0] = checks, r32 = the digest r was reduced from.
extern "C" void hs_locate_points_host(uint8_t *ok, uint8_t *status, uint64_t *stats, uint8_t *r32, const uint8_t *c48,
                                      const uint8_t *z32, const uint8_t *y32, const uint8_t *p48, uint64_t n,
                                      const G2Jac *tau_g2, int64_t max_checks) {
    G2Prepared q1, q2;
    g2_prepare(q1, g2_to_affine(g2_generator()));
    g2_prepare(q2, g2_to_affine(*tau_g2));
    auto fr_canonical = [](uint32_t raw[8], const uint8_t *b) {
        uint32_t m[8];
        for (int i = 0; i < 8; i++) {
            const uint8_t *p = b + 4 * (7 - i);
            raw[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
        }
        mod_limbs<FrParams>(m);
        return !limbs_geq<8>(raw, m);
    };
    locate_point_digest<Sha256>(r32, c48, z32, y32, p48, n);
    uint32_t rraw[8];
    for (int i = 0; i < 8; i++) {
        const uint8_t *p = r32 + 4 * (7 - i);
        rraw[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
    const Fr r = from_raw<FrParams>(rraw);   // (reduces)
    std::vector<uint8_t> invalid(n ? n : 1), okb(n ? n : 1);
    std::vector<G1Jac> pa(n + 1), pb(n + 1);   // PA[0] = PB[0] = infinity
    pa[0] = pb[0] = G1Jac::inf();
    Fr rp = Fr::one();
    for (uint64_t i = 0; i < n; i++, rp = mul(rp, r)) {
        G1Affine c, pr;
        uint32_t z[8], y[8], k[8];
        bool bad = g1_uncompress(c, c48 + 48 * i) != 0 || g1_uncompress(pr, p48 + 48 * i) != 0;
        bad = bad || !g1_in_subgroup_host(c) || !g1_in_subgroup_host(pr);
        bad = !fr_canonical(z, z32 + 32 * i) || bad;
        bad = !fr_canonical(y, y32 + 32 * i) || bad;
        invalid[i] = bad ? 1 : 0;
        G1Jac a = G1Jac::inf(), b = G1Jac::inf();
        if (!bad) {
            const G1Jac proof = jac_from_affine(pr);
            const G1Jac p1 = jac_add(jac_add(jac_from_affine(c), jac_neg(g1_mul_glv_host(g1_generator(), y))), g1_mul_glv_host(proof, z));
            to_raw<FrParams>(k, rp);
            a = g1_mul_glv_host(p1, k);
            b = g1_mul_glv_host(proof, k);
        }
        pa[i + 1] = jac_add(pa[i], a);
        pb[i + 1] = jac_add(pb[i], b);
    }
    auto range_ok = [&](size_t lo, size_t hi) {
        const G1Jac da = jac_add(pa[hi], jac_neg(pa[lo])), db = jac_add(pb[hi], jac_neg(pb[lo]));
        return pairing_product_is_one(jac_to_affine(da), q1, jac_to_affine(jac_neg(db)), q2);
    };
    auto serial = [](size_t m, auto &&fn) {
        for (size_t i = 0; i < m; i++) fn(i);
    };
    const LocateOutcome res = locate_bisect(reinterpret_cast<bool *>(okb.data()), invalid.data(), (size_t)n,
                                            max_checks < 0 ? UINT64_MAX : (uint64_t)max_checks, range_ok, serial);
    for (uint64_t i = 0; i < n; i++) {
        ok[i] = okb[i];
        status[i] = invalid[i];
    }
    stats[0] = res.checks;
    stats[1] = res.open.size();
}

// ---- ckzg_hip_verify_cell_kzg_proof_batch_locate: the chunk's two-level digest, and the whole second half in host
// arithmetic (tests/test_cell_locate_cpu.py). ----
#include <map>
#include <string>
extern "C" void hs_locate_cell_digest(uint8_t *digest32, const uint8_t *c48, const uint64_t *cell_indices, const uint8_t *cells,
                                      const uint8_t *p48, uint64_t n) {
    locate_cell_digest<Sha256>(digest32, c48, cell_indices, cells, p48, n);
}

// Per item: validation (index < 128, 64 canonical field elements, both points in G1), the interpolation polynomial of
// the cell over its coset by the definition of the inverse transform (64 x 64 products, no butterflies: a route of its
// own), P1_i = C_i - sum_k I_i[k] mono64[k] + [h_i^64] proof_i, then as hs_locate_points_host: r from
// locate_cell_digest, A_i = [r^i] P1_i, B_i = [r^i] proof_i, prefix sums and the bisection over
// e(PA[b] - PA[a], [1]_2) * e(-(PB[b] - PB[a]), [s^64]_2) == 1.  mono48: g1_values_monomial[0..63] as the setup file has
// them (64 x 48 bytes), s64_g2: [s^64]_2.  Out: ok[n], status[n] (1 = invalid item), stats[0] = checks, stats[1] = ranges
// left open, r32 = the digest r was reduced from.  Returns 0, or 1 if a setup point does not decompress.
extern "C" int hs_locate_cells_host(uint8_t *ok, uint8_t *status, uint64_t *stats, uint8_t *r32, const uint8_t *c48,
                                    const uint64_t *cell_indices, const uint8_t *cells, const uint8_t *p48, uint64_t n,
                                    const uint8_t *mono48, const G2Jac *s64_g2, int64_t max_checks) {
    G2Prepared q1, q2;
    g2_prepare(q1, g2_to_affine(g2_generator()));
    g2_prepare(q2, g2_to_affine(*s64_g2));
    G1Jac mono[64];
    for (int k = 0; k < 64; k++) {
        G1Affine a;
        if (g1_uncompress(a, mono48 + 48 * k) != 0) return 1;
        mono[k] = jac_from_affine(a);
    }
    // w = 7^((r - 1) / 8192), the 8192-th root of unity the setup uses; roots[i] = w^i
    std::vector<Fr> roots(8192);
    {
        uint32_t e[8], seven[8] = {7, 0, 0, 0, 0, 0, 0, 0};
        mod_limbs<FrParams>(e);
        e[0] -= 1;   // (r is odd)
        for (int i = 0; i < 8; i++) e[i] = (e[i] >> 13) | (i < 7 ? e[i + 1] << 19 : 0u);
        Fr w = Fr::one(), base = from_raw<FrParams>(seven);
        for (int i = 0; i < 256; i++, base = mul(base, base))
            if ((e[i >> 5] >> (i & 31)) & 1u) w = mul(w, base);
        roots[0] = Fr::one();
        for (int i = 1; i < 8192; i++) roots[i] = mul(roots[i - 1], w);
    }
    uint32_t sixty_four[8] = {64, 0, 0, 0, 0, 0, 0, 0};
    const Fr inv64 = fr_inv_safegcd(from_raw<FrParams>(sixty_four));
    auto brp = [](uint32_t v, int bits) {
        uint32_t o = 0;
        for (int b = 0; b < bits; b++) o |= ((v >> b) & 1u) << (bits - 1 - b);
        return o;
    };
    locate_cell_digest<Sha256>(r32, c48, cell_indices, cells, p48, n);
    uint32_t rraw[8];
    for (int i = 0; i < 8; i++) {
        const uint8_t *p = r32 + 4 * (7 - i);
        rraw[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
    const Fr r = from_raw<FrParams>(rraw);   // (reduces)
    std::vector<uint8_t> invalid(n ? n : 1), okb(n ? n : 1);
    std::vector<G1Jac> pa(n + 1), pb(n + 1);   // PA[0] = PB[0] = infinity
    pa[0] = pb[0] = G1Jac::inf();
    std::map<std::string, G1Jac> interp_of;   // [I(s)]_1 per distinct (column, cell): the vectors repeat their cells
    Fr rp = Fr::one();
    for (uint64_t i = 0; i < n; i++, rp = mul(rp, r)) {
        G1Affine c, pr;
        bool bad = g1_uncompress(c, c48 + 48 * i) != 0 || g1_uncompress(pr, p48 + 48 * i) != 0;
        bad = bad || !g1_in_subgroup_host(c) || !g1_in_subgroup_host(pr);
        bad = bad || cell_indices[i] >= 128;
        Fr ev[64];
        for (int j = 0; j < 64 && !bad; j++) {
            uint32_t raw[8], m[8];
            for (int w = 0; w < 8; w++) {
                const uint8_t *p = cells + 2048 * i + 32 * j + 4 * (7 - w);
                raw[w] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            }
            mod_limbs<FrParams>(m);
            bad = limbs_geq<8>(raw, m);
            ev[j] = from_raw<FrParams>(raw);
        }
        invalid[i] = bad ? 1 : 0;
        G1Jac a = G1Jac::inf(), b = G1Jac::inf();
        if (!bad) {
            const uint32_t rb = brp((uint32_t)cell_indices[i], 7);
            std::string key(reinterpret_cast<const char *>(cells + 2048 * i), 2048);
            key.push_back((char)cell_indices[i]);
            auto it = interp_of.find(key);
            if (it == interp_of.end()) {
                G1Jac sum = G1Jac::inf();
                for (uint32_t k = 0; k < 64; k++) {
                    // coefficient k of the polynomial through ev[brp6(j)] at h w64^j: (1/64) sum_j ev[brp6(j)] w64^(-jk), times h^-k
                    Fr ck = Fr::zero();
                    for (uint32_t j = 0; j < 64; j++) ck = add(ck, mul(ev[brp(j, 6)], roots[(8192u - 128u * ((j * k) & 63u)) & 8191u]));
                    ck = mul(mul(ck, inv64), roots[((8192u - rb) * k) & 8191u]);
                    uint32_t kraw[8];
                    to_raw<FrParams>(kraw, ck);
                    sum = jac_add(sum, g1_mul_glv_host(mono[k], kraw));
                }
                it = interp_of.emplace(key, sum).first;
            }
            uint32_t h64[8], k[8];
            to_raw<FrParams>(h64, roots[64u * rb]);
            const G1Jac proof = jac_from_affine(pr);
            const G1Jac p1 = jac_add(jac_add(jac_from_affine(c), jac_neg(it->second)), g1_mul_glv_host(proof, h64));
            to_raw<FrParams>(k, rp);
            a = g1_mul_glv_host(p1, k);
            b = g1_mul_glv_host(proof, k);
        }
        pa[i + 1] = jac_add(pa[i], a);
        pb[i + 1] = jac_add(pb[i], b);
    }
    auto range_ok = [&](size_t lo, size_t hi) {
        const G1Jac da = jac_add(pa[hi], jac_neg(pa[lo])), db = jac_add(pb[hi], jac_neg(pb[lo]));
        return pairing_product_is_one(jac_to_affine(da), q1, jac_to_affine(jac_neg(db)), q2);
    };
    auto serial = [](size_t m, auto &&fn) {
        for (size_t i = 0; i < m; i++) fn(i);
    };
    const LocateOutcome res = locate_bisect(reinterpret_cast<bool *>(okb.data()), invalid.data(), (size_t)n,
                                            max_checks < 0 ? UINT64_MAX : (uint64_t)max_checks, range_ok, serial);
    for (uint64_t i = 0; i < n; i++) {
        ok[i] = okb[i];
        status[i] = invalid[i];
    }
    stats[0] = res.checks;
    stats[1] = res.open.size();
    return 0;
}

// ---- ckzg_hip_verify_coset_kzg_proof_batch_locate: the cell form's two functions at every coset size l = 2^e, e <= 6
// (tests/test_coset_locate_cpu.py), and the launch plan of the call (coset_locate_plan.hpp). ----
#include "coset_locate_plan.hpp"
extern "C" void hs_locate_coset_digest(uint8_t *digest32, const uint8_t *c48, const uint64_t *coset_indices, const uint8_t *evals,
                                       const uint8_t *p48, uint64_t n, int e) {
    locate_coset_digest<Sha256>(digest32, c48, coset_indices, evals, p48, n, e);
}
extern "C" uint64_t hs_coset_locate_chunk_items(int e) { return coset_locate_chunk_items(e); }
extern "C" int hs_coset_locate_sum_lpv(int e, uint64_t items) { return coset_locate_sum_lpv(e, items); }
// what[0 .. 6] = COSET_LOCATE_SUM_WAVE_BELOW, what[7 .. 13] = COSET_LOCATE_SUM_LPV, what[14] = smallest shard
extern "C" void hs_coset_locate_constants(uint64_t *what) {
    for (int e = 0; e <= COSET_MAX_LOG; e++) {
        what[e] = COSET_LOCATE_SUM_WAVE_BELOW[e];
        what[7 + e] = (uint64_t)COSET_LOCATE_SUM_LPV[e];
    }
    what[14] = COSET_LOCATE_MIN_SHARD;
}

// Per item: validation (index < m = 8192 >> e, l canonical values, both points in G1), the interpolation polynomial of
// the item's values over its coset by the definition of the inverse transform (l x l products, no butterflies: a route
// of its own) -- a_k = x_c^-k (1/l) sum_j y_j w_l^(-brp_e(j) k), x_c = w^brp_{13-e}(c) -- then
// P1_i = C_i - sum_k a_k mono[k] + [x_c^l] proof_i and, as hs_locate_cells_host, r from locate_coset_digest,
// A_i = [r^i] P1_i, B_i = [r^i] proof_i, prefix sums and the bisection over
// e(PA[b] - PA[a], [1]_2) * e(-(PB[b] - PB[a]), [s^l]_2) == 1.  mono48: g1_values_monomial[0 .. l - 1] as the setup file
// has them, sl_g2: [s^l]_2 = g2_values_monomial[l].  Out as hs_locate_cells_host.  Returns 0, 1 if a setup point does
// not decompress, 2 for e out of range.
extern "C" int hs_locate_cosets_host(uint8_t *ok, uint8_t *status, uint64_t *stats, uint8_t *r32, const uint8_t *c48,
                                     const uint64_t *coset_indices, const uint8_t *evals, const uint8_t *p48, uint64_t n, int e,
                                     const uint8_t *mono48, const G2Jac *sl_g2, int64_t max_checks) {
    if (e < 0 || e > COSET_MAX_LOG) return 2;
    const uint32_t l = 1u << e, m = 8192u >> e;
    G2Prepared q1, q2;
    g2_prepare(q1, g2_to_affine(g2_generator()));
    g2_prepare(q2, g2_to_affine(*sl_g2));
    G1Jac mono[64];
    for (uint32_t k = 0; k < l; k++) {
        G1Affine a;
        if (g1_uncompress(a, mono48 + 48 * k) != 0) return 1;
        mono[k] = jac_from_affine(a);
    }
    // w = 7^((r - 1) / 8192), the 8192-th root of unity the setup uses; roots[i] = w^i
    std::vector<Fr> roots(8192);
    {
        uint32_t ex[8], seven[8] = {7, 0, 0, 0, 0, 0, 0, 0};
        mod_limbs<FrParams>(ex);
        ex[0] -= 1;   // (r is odd)
        for (int i = 0; i < 8; i++) ex[i] = (ex[i] >> 13) | (i < 7 ? ex[i + 1] << 19 : 0u);
        Fr w = Fr::one(), base = from_raw<FrParams>(seven);
        for (int i = 0; i < 256; i++, base = mul(base, base))
            if ((ex[i >> 5] >> (i & 31)) & 1u) w = mul(w, base);
        roots[0] = Fr::one();
        for (int i = 1; i < 8192; i++) roots[i] = mul(roots[i - 1], w);
    }
    uint32_t lraw[8] = {l, 0, 0, 0, 0, 0, 0, 0};
    const Fr inv_l = fr_inv_safegcd(from_raw<FrParams>(lraw));
    auto brp = [](uint32_t v, int bits) {
        uint32_t o = 0;
        for (int b = 0; b < bits; b++) o |= ((v >> b) & 1u) << (bits - 1 - b);
        return o;
    };
    locate_coset_digest<Sha256>(r32, c48, coset_indices, evals, p48, n, e);
    uint32_t rraw[8];
    for (int i = 0; i < 8; i++) {
        const uint8_t *p = r32 + 4 * (7 - i);
        rraw[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
    const Fr r = from_raw<FrParams>(rraw);   // (reduces)
    std::vector<uint8_t> invalid(n ? n : 1), okb(n ? n : 1);
    std::vector<G1Jac> pa(n + 1), pb(n + 1);   // PA[0] = PB[0] = infinity
    pa[0] = pb[0] = G1Jac::inf();
    Fr rp = Fr::one();
    for (uint64_t i = 0; i < n; i++, rp = mul(rp, r)) {
        G1Affine c, pr;
        bool bad = g1_uncompress(c, c48 + 48 * i) != 0 || g1_uncompress(pr, p48 + 48 * i) != 0;
        bad = bad || !g1_in_subgroup_host(c) || !g1_in_subgroup_host(pr);
        bad = bad || coset_indices[i] >= m;
        Fr ev[64];
        for (uint32_t j = 0; j < l && !bad; j++) {
            uint32_t raw[8], md[8];
            for (int w = 0; w < 8; w++) {
                const uint8_t *p = evals + 32 * ((size_t)i * l + j) + 4 * (7 - w);
                raw[w] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            }
            mod_limbs<FrParams>(md);
            bad = limbs_geq<8>(raw, md);
            ev[j] = from_raw<FrParams>(raw);
        }
        invalid[i] = bad ? 1 : 0;
        G1Jac a = G1Jac::inf(), b = G1Jac::inf();
        if (!bad) {
            const uint32_t rb = brp((uint32_t)coset_indices[i], 13 - e);   // x_c = w^rb
            G1Jac sum = G1Jac::inf();
            for (uint32_t k = 0; k < l; k++) {
                // value j sits at x_c w_l^brp_e(j), w_l = w^(8192 / l)
                Fr ck = Fr::zero();
                for (uint32_t j = 0; j < l; j++) ck = add(ck, mul(ev[j], roots[(8192u - m * ((brp(j, e) * k) & (l - 1u))) & 8191u]));
                ck = mul(mul(ck, inv_l), roots[((8192u - rb) * k) & 8191u]);
                uint32_t kraw[8];
                to_raw<FrParams>(kraw, ck);
                sum = jac_add(sum, g1_mul_glv_host(mono[k], kraw));
            }
            uint32_t xl[8], k[8];
            to_raw<FrParams>(xl, roots[(rb << e) & 8191u]);
            const G1Jac proof = jac_from_affine(pr);
            const G1Jac p1 = jac_add(jac_add(jac_from_affine(c), jac_neg(sum)), g1_mul_glv_host(proof, xl));
            to_raw<FrParams>(k, rp);
            a = g1_mul_glv_host(p1, k);
            b = g1_mul_glv_host(proof, k);
        }
        pa[i + 1] = jac_add(pa[i], a);
        pb[i + 1] = jac_add(pb[i], b);
    }
    auto range_ok = [&](size_t lo, size_t hi) {
        const G1Jac da = jac_add(pa[hi], jac_neg(pa[lo])), db = jac_add(pb[hi], jac_neg(pb[lo]));
        return pairing_product_is_one(jac_to_affine(da), q1, jac_to_affine(jac_neg(db)), q2);
    };
    auto serial = [](size_t cnt, auto &&fn) {
        for (size_t i = 0; i < cnt; i++) fn(i);
    };
    const LocateOutcome res = locate_bisect(reinterpret_cast<bool *>(okb.data()), invalid.data(), (size_t)n,
                                            max_checks < 0 ? UINT64_MAX : (uint64_t)max_checks, range_ok, serial);
    for (uint64_t i = 0; i < n; i++) {
        ok[i] = okb[i];
        status[i] = invalid[i];
    }
    stats[0] = res.checks;
    stats[1] = res.open.size();
    return 0;
}

// ---- g1_fft_plan.hpp: the index maps, the form picker and the chunk split of the general G1 transform and of the
// ---- openings at every domain point (tests/test_domain_openings_cpu.py) ----
#include "g1_fft_plan.hpp"

extern "C" int hs_g1_fft_log2(uint64_t n) { return g1_fft_log2(n); }
extern "C" uint32_t hs_g1_fft_ladders(int logn, int s) { return g1_fft_ladders(logn, s); }
extern "C" void hs_g1_fft_ladder_index(uint32_t m, int s, uint32_t *i1, uint32_t *root) { g1_fft_ladder_index(m, s, *i1, *root); }
extern "C" int hs_g1_fft_form(uint64_t products, uint64_t quad_max) { return g1_fft_form(products, quad_max); }
extern "C" int hs_g1_fft_form_at(int logn, uint64_t count, uint64_t quad_max) { return g1_fft_form_at(logn, count, quad_max); }
extern "C" uint64_t hs_g1_fft_quad_max_default() { return G1_FFT_QUAD_MAX_DEFAULT; }
extern "C" uint64_t hs_domain_chunk_count(uint64_t n, uint64_t chunk) { return domain_chunk_count(n, chunk); }
extern "C" uint64_t hs_domain_chunk_size(uint64_t n, uint64_t chunk, uint64_t c) { return domain_chunk_size(n, chunk, c); }

// ---- the maps of the openings, every coset size (tests/test_coset_openings_cpu.py, tests/test_domain_openings_cpu.py) ----
extern "C" int hs_coset_max_log() { return COSET_MAX_LOG; }
extern "C" uint32_t hs_coset_proofs_per_blob(int e) { return coset_proofs_per_blob(e); }
extern "C" int hs_coset_circulant_source(uint32_t t, int e, uint32_t n) { return coset_circulant_source(t, e, n); }
extern "C" int hs_coset_setup_source(uint32_t t, int e, uint32_t n) { return coset_setup_source(t, e, n); }
extern "C" uint32_t hs_coset_colsum_radix() { return COSET_COLSUM_RADIX; }
extern "C" uint32_t hs_coset_colsum_parts(int e) { return coset_colsum_parts(e); }

// ---- fk20_fft_plan.hpp: which form the two G1 transforms of FK20 take for n transforms, at the default hand-over
// ---- points (tests/test_fk20_expect_cpu.py) ----
#include "fk20_fft_plan.hpp"
extern "C" int hs_fk20_fft_form(uint64_t n) { return fk20_fft_form(n); }
extern "C" uint64_t hs_fk20_fft_scratch_bytes(uint64_t n) { return fk20_fft_scratch_plan(n, fk20_fft_form(n)).bytes; }

// ---- coset multiproof verification, every coset size (tests/test_coset_verify_cpu.py) ----
#include "coset_verify_plan.hpp"
extern "C" uint32_t hs_coset_verify_cosets(int e) { return coset_verify_cosets(e); }
extern "C" uint32_t hs_coset_verify_brp(uint32_t c, int e) { return coset_verify_brp(c, e); }
extern "C" uint32_t hs_coset_verify_shift_root(uint32_t c, int e) { return coset_verify_shift_root(c, e); }
extern "C" uint32_t hs_coset_verify_unshift_root(uint32_t c, int e, uint32_t k) { return coset_verify_unshift_root(c, e, k); }
extern "C" uint32_t hs_coset_verify_slot(uint32_t c, int e, uint32_t j) { return coset_verify_slot(c, e, j); }
extern "C" uint32_t hs_coset_verify_twiddle_root(uint32_t pos, int s) { return coset_verify_twiddle_root(pos, s); }
extern "C" uint32_t hs_coset_verify_agg_parts(uint64_t items, int e) { return coset_verify_agg_parts(items, e); }
// what[0] = items per lane, [1] = most parts, [2] = transcript on the pool from, [3] = smallest shard, [4] = slots per
// aggregation workgroup, [5] = threads of an interpolation workgroup
extern "C" void hs_coset_verify_constants(uint64_t *what) {
    what[0] = COSET_AGG_ITEMS_PER_LANE;
    what[1] = COSET_AGG_MAX_PARTS;
    what[2] = COSET_VERIFY_HASH_ON_POOL_FROM;
    what[3] = COSET_VERIFY_MIN_SHARD;
    what[4] = COSET_AGG_SLOTS_PER_BLOCK;
    what[5] = COSET_INTERP_THREADS;
}
extern "C" void hs_coset_verify_digest(uint8_t *digest32, const uint8_t *commitments48, uint64_t num_commitments,
                                       const uint64_t *commitment_indices, const uint64_t *coset_indices,
                                       const uint8_t *evals32, const uint8_t *proofs48, uint64_t num_cosets, int e) {
    coset_verify_digest<Sha256>(digest32, commitments48, num_commitments, commitment_indices, coset_indices, evals32, proofs48,
                                num_cosets, e);
}

// ---- recovery from untrusted cosets: the planning of the repair pass (coset_repair_plan.hpp) replayed from flags the
// caller makes up (tests/test_coset_repair_cpu.py, whose model is tests/coset_repair_expect.py).  One call is one shard
// [0, num_rows): first-pass flags status / high1 / mismatch1 [num_rows]; with_proofs != 0: the locate pass runs, item_ok
// being its answers at the CALLER'S flat cosets (read only at the located rows' cosets); high2 / mismatch2 [num_rows]:
// the second pass's flags at the caller rows it lands on.  Out: verdict [num_rows], coset_ok [cosets] (may be null),
// loc_rows [num_rows], item_src / item_row [cosets], out_row [num_rows], start2 [num_rows + 1], src2 [cosets], lost
// [num_rows]; counts[5] = located rows, items, second-pass rows, cosets of the second pass, lost rows.  Returns 0, or -1
// for e > 6 or a malformed row_start. ----
#include <algorithm>
#include "coset_repair_plan.hpp"
extern "C" long hs_coset_repair_plan(uint8_t *verdict, uint8_t *coset_ok, uint64_t *loc_rows, uint64_t *item_src, uint64_t *item_row,
                                     uint64_t *out_row, uint64_t *start2, uint64_t *src2, uint64_t *lost, uint64_t *counts,
                                     const uint8_t *status, const uint8_t *high1, const uint8_t *mismatch1, const uint8_t *item_ok,
                                     const uint8_t *high2, const uint8_t *mismatch2, const uint64_t *row_start, uint64_t num_rows,
                                     int with_proofs, int e) {
    if (e < 0 || e > 6 || !slice_starts_ok(row_start, num_rows)) return -1;
    const uint64_t total = row_start[num_rows];
    std::unique_ptr<bool[]> ok(new bool[total ? total : 1]), cok(new bool[total ? total : 1]);
    coset_repair_first_pass(verdict, coset_ok ? cok.get() : nullptr, status, high1, mismatch1, row_start, 0, num_rows);
    for (int j = 0; j < 5; j++) counts[j] = 0;
    start2[0] = 0;
    if (with_proofs) {
        CosetRepairLocate lp;
        coset_repair_locate_plan(lp, verdict, row_start, 0, num_rows);
        for (size_t i = 0; i < lp.items(); i++) ok[i] = item_ok[lp.item_src[i]] != 0;
        if (coset_ok) coset_repair_spread_ok(cok.get(), lp, ok.get());
        CosetRepairSecond sp;
        coset_repair_second_plan(sp, lp, ok.get(), e);
        coset_repair_lost(verdict, sp);
        coset_repair_finish(verdict, sp, high2, mismatch2);
        counts[0] = lp.rows.size(), counts[1] = lp.items(), counts[2] = sp.rows(), counts[3] = sp.src.size(), counts[4] = sp.lost.size();
        std::copy(lp.rows.begin(), lp.rows.end(), loc_rows);
        std::copy(lp.item_src.begin(), lp.item_src.end(), item_src);
        std::copy(lp.item_row.begin(), lp.item_row.end(), item_row);
        std::copy(sp.out_row.begin(), sp.out_row.end(), out_row);
        std::copy(sp.row_start.begin(), sp.row_start.end(), start2);
        std::copy(sp.src.begin(), sp.src.end(), src2);
        std::copy(sp.lost.begin(), sp.lost.end(), lost);
    }
    if (coset_ok)
        for (uint64_t i = 0; i < total; i++) coset_ok[i] = cok[i] ? 1 : 0;
    return 0;
}

// ---- Fp on 13 signed 30-bit limbs (fp30.hpp) and the accumulate loop's mixed addition on it (g1_30.hpp) ----
#include "f30_test_ops.hpp"
namespace {
template <int V>
F30<1, V> f30_load(const int32_t *a) {
    F30<1, V> r;
    for (int j = 0; j < 13; j++) r.l[j] = a[j];
    return r;
}
template <int L, int V>
void f30_store(int32_t *r, const F30<L, V> &a) {
    for (int j = 0; j < 13; j++) r[j] = a.l[j];
}
Fp table_words(const Fp &v) {   // a table coordinate as msm.hip gathers it: 2^392 domain, fully reduced, packed
    Fp k;
    for (int i = 0; i < 12; i++) k.l[i] = FP_MONT_2POW8[i];
    return mul(v, k);
}
}  // namespace
extern "C" {
// limbs in, limbs out, at the widest value bounds the static_asserts admit (17 * 18, 17^2, 17 * 17 + 5 * 5)
void hs_fp30_mul(int32_t *r, const int32_t *a, const int32_t *b) { f30_store(r, mul(f30_load<17>(a), f30_load<18>(b))); }
void hs_fp30_sqr(int32_t *r, const int32_t *a) { f30_store(r, sqr(f30_load<17>(a))); }
void hs_fp30_mul_add2(int32_t *r, const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d) {
    f30_store(r, mul_add2(f30_load<17>(a), f30_load<17>(b), f30_load<5>(c), f30_load<5>(d)));
}
// limbs of up to 3 * 2^29 in magnitude
void hs_fp30_norm(int32_t *r, const int32_t *a) {
    F30<3, 200> x;
    for (int j = 0; j < 13; j++) x.l[j] = a[j];
    f30_store(r, norm(x));
}
void hs_fp30_add(int32_t *r, const int32_t *a, const int32_t *b) { f30_store(r, add(f30_load<1>(a), f30_load<1>(b))); }
void hs_fp30_sub(int32_t *r, const int32_t *a, const int32_t *b) { f30_store(r, sub(f30_load<1>(a), f30_load<1>(b))); }
void hs_fp30_unpack(int32_t *r, const uint32_t *w) { f30_store(r, f30_unpack(w)); }
void hs_fp30_to_f28(uint32_t *r, const int32_t *a) {
    auto o = f30_to_f28(f30_load<1>(a));
    for (int j = 0; j < 14; j++) r[j] = o.l[j];
}
void hs_fp30_consts(int32_t *p, uint32_t *ninv, int32_t *r392, int32_t *r394, int32_t *beta390) {
    for (int j = 0; j < 13; j++) p[j] = F30_P[j], r392[j] = F30_R392[j], r394[j] = F30_R394[j], beta390[j] = F30_BETA390[j];
    *ninv = F30_NINV;
}
// f30_test_ops.hpp as g++ builds it: operation `op` of the list on n items (13 int32 per operand, 14 words per result)
const char *hs_f30_ops() { return f30test::desc(); }
int hs_f30_run(int op, int32_t *out, const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int n) {
    for (int i = 0; i < n; i++)
        if (!f30test::run(op, out + 14 * i, a + 13 * i, b + 13 * i, c + 13 * i, d + 13 * i)) return 1;
    return 0;
}
// the addition on raw state (f30_test_ops.hpp): per item 52 int32 of state, flags (inf, yneg, dneg) in and (inf, yneg) out,
// a 24-word table entry
void hs_madd30_step(int32_t *out, uint8_t *oflags, const int32_t *state, const uint8_t *flags, const uint32_t *entry, int n) {
    for (int i = 0; i < n; i++)
        f30test::madd_step(out + f30test::STATE_WORDS * i, oflags + 2 * i, state + f30test::STATE_WORDS * i, flags + 3 * i,
                           entry + f30test::ENTRY_WORDS * i);
}
void hs_phi30(int32_t *out, const int32_t *state, int n) {
    for (int i = 0; i < n; i++) f30test::phi_step(out + f30test::STATE_WORDS * i, state + f30test::STATE_WORDS * i);
}
void hs_exit30(uint32_t *out, uint8_t *met, const int32_t *state, int n) {
    for (int i = 0; i < n; i++) f30test::exit_step(out + f30test::EXIT_WORDS * i, met + i, state + f30test::STATE_WORDS * i);
}
// One lane's chain of the accumulate loop: entries pts[i] (skipped where at_inf[i]), negated where signs[i], phi applied
// before entry phi_at (phi_at >= n: at the end).  form 0: the 28-bit law (xyzz28_madd_alt), the reference of the two
// others.  form 1: the 30-bit law through entry and exit, as it stands.  form 2: what msm_sum_pairs30's caller does --
// the 30-bit law, and the 28-bit one again if the exit finds ZZ = 0.  Returns the exit's equal-x verdict (form 0: 0).
int hs_g1_madd_alt_chain_form(G1Jac *r, const G1Affine *pts, const uint8_t *signs, const uint8_t *at_inf, int n, int phi_at,
                              int form) {
    auto run28 = [&](XYZZ28 &acc, bool &inf, bool &yneg) {
        inf = true, yneg = false;
        bool phi_pending = true;
        for (int i = 0; i < n; i++) {
            if (phi_pending && i >= phi_at) {
                if (!inf) acc.x = widen<1, 10>(mul(acc.x, f28_const<1, 1>(FP28_BETA_LAMBDA)));
                phi_pending = false;
            }
            if (at_inf[i]) continue;
            xyzz28_madd_alt(acc, inf, yneg, table_coord(pts[i].x), table_coord(pts[i].y), signs[i] != 0);
        }
        if (phi_pending && !inf) acc.x = widen<1, 10>(mul(acc.x, f28_const<1, 1>(FP28_BETA_LAMBDA)));
    };
    XYZZ28 acc28;
    bool inf = true, yneg = false;
    int met = 0;
    if (form == 0) {
        run28(acc28, inf, yneg);
    } else {
        XYZZ30 acc;
        bool phi_pending = true;
        for (int i = 0; i < n; i++) {
            if (phi_pending && i >= phi_at) {
                if (!inf) xyzz30_apply_phi(acc);
                phi_pending = false;
            }
            if (at_inf[i]) continue;
            Fp x = table_words(pts[i].x), y = table_words(pts[i].y);
            xyzz30_madd_alt(acc, inf, yneg, f30_unpack(x.l), f30_unpack(y.l), signs[i] != 0);
        }
        if (phi_pending && !inf) xyzz30_apply_phi(acc);
        if (!inf) {
            acc28 = xyzz30_to_xyzz28(acc);
            met = xyzz30_met_equal_x(acc28) ? 1 : 0;
        }
        if (met && form == 2) run28(acc28, inf, yneg);
    }
    xyzz28_fix_sign(acc28, inf, yneg);
    *r = jac_from_xyzz(xyzz28_to_xyzz(acc28, inf));
    return met;
}
}
