// pairing_dev.hpp -- the BLS12-381 pairing check against two FIXED G2 arguments, for one lane of a GPU kernel
// (pairing.hip: k_pairing_check) and, compiled by g++, for the host shim that tests it (host_shim.cpp).
//
// The formulas are those of host_pairing.hpp -- the tower Fp2 = Fp[u]/(u^2+1), Fp6 = Fp2[v]/(v^3-(1+u)),
// Fp12 = Fp6[w]/(w^2-v), the sparse product by a prepared line, the two-pair Miller product that shares its squarings,
// the final exponentiation (easy part with ONE fp_inv, hard part through Granger-Scott squarings and pow_x) -- restated
// on field.hpp's host/device Mont<FpParams>.  host_pairing.hpp keeps the host's lazily reduced 64-bit forms and is the
// reference this header is tested against (tests/test_point_pairing_host.py): every value here is fully reduced, so
// the two agree byte for byte.  The types have host_pairing.hpp's layout, so the lam[] and c[] arrays of its G2Prepared
// line tables are copied to the device as they are.
//
// Code size: an Fp12 is 144 VGPRs; with every product force-inlined one pairing is hundreds of thousands of
// instructions.  The Fp2 / Fp6 / Fp12 products and squares, the line product, pow_x and the inversions are therefore
// out-of-line device functions (PD_CALL); only the Fp product (field.hpp) and the cheap add / sub / select forms are
// inlined into them.
#pragma once
#include "g1.hpp"

#if defined(__HIPCC__)
#define PD_CALL HDNI __attribute__((noinline))
#else
#define PD_CALL inline
#endif

namespace ckzg {
namespace pdev {

constexpr int MILLER_STEPS = 68;  // 63 doublings + 5 additions for |x| = 0xd201000000010000 (host_pairing.hpp)

struct Fp2 {
    Fp c0, c1;
};
struct Fp6 {
    Fp2 c0, c1, c2;
};
struct Fp12 {
    Fp6 c0, c1;
};
// one step of a prepared line: the slope and lam * x_T - y_T
struct LineCoeffs {
    Fp2 lam, c;
};
// A prepared G2 argument: host_pairing.hpp's G2Prepared::lam[MILLER_STEPS] and ::c[MILLER_STEPS] as they are (in HBM on
// the device, read by every lane of a wave at the same step).
struct LineTable {
    const Fp2 *lam, *c;
    HD LineCoeffs operator()(int n) const { return {lam[n], c[n]}; }
};

// ---- Fp2 ----
HD Fp2 add(const Fp2 &a, const Fp2 &b) { return {add(a.c0, b.c0), add(a.c1, b.c1)}; }
HD Fp2 sub(const Fp2 &a, const Fp2 &b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
HD Fp2 neg(const Fp2 &a) { return {neg(a.c0), neg(a.c1)}; }
HD Fp2 dbl(const Fp2 &a) { return add(a, a); }
HD Fp2 mul_xi(const Fp2 &a) { return {sub(a.c0, a.c1), add(a.c0, a.c1)}; }  // * (1+u)
HD Fp2 conj(const Fp2 &a) { return {a.c0, neg(a.c1)}; }
// Karatsuba: 3 base-field products
PD_CALL Fp2 mul(const Fp2 &a, const Fp2 &b) {
    const Fp t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);
    const Fp t2 = mul(add(a.c0, a.c1), add(b.c0, b.c1));
    return {sub(t0, t1), sub(sub(t2, t0), t1)};
}
PD_CALL Fp2 sqr(const Fp2 &a) {
    const Fp m = mul(a.c0, a.c1);
    return {mul(add(a.c0, a.c1), sub(a.c0, a.c1)), dbl(m)};
}
HD Fp2 mul_fp(const Fp2 &a, const Fp &k) { return {mul(a.c0, k), mul(a.c1, k)}; }
PD_CALL Fp2 inv(const Fp2 &a) {
    const Fp n = fp_inv(add(sqr(a.c0), sqr(a.c1)));
    return {mul(a.c0, n), neg(mul(a.c1, n))};
}

// ---- Fp6 ----
HD Fp6 add(const Fp6 &a, const Fp6 &b) { return {add(a.c0, b.c0), add(a.c1, b.c1), add(a.c2, b.c2)}; }
HD Fp6 sub(const Fp6 &a, const Fp6 &b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1), sub(a.c2, b.c2)}; }
HD Fp6 neg(const Fp6 &a) { return {neg(a.c0), neg(a.c1), neg(a.c2)}; }
HD Fp6 mul_v(const Fp6 &a) { return {mul_xi(a.c2), a.c0, a.c1}; }
PD_CALL Fp6 mul(const Fp6 &a, const Fp6 &b) {
    const Fp2 v0 = mul(a.c0, b.c0), v1 = mul(a.c1, b.c1), v2 = mul(a.c2, b.c2);
    const Fp2 t12 = sub(sub(mul(add(a.c1, a.c2), add(b.c1, b.c2)), v1), v2);  // a1b2 + a2b1
    const Fp2 t01 = sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), v0), v1);  // a0b1 + a1b0
    const Fp2 t02 = sub(sub(mul(add(a.c0, a.c2), add(b.c0, b.c2)), v0), v2);  // a0b2 + a2b0
    return {add(v0, mul_xi(t12)), add(t01, mul_xi(v2)), add(t02, v1)};
}
PD_CALL Fp6 inv(const Fp6 &a) {
    const Fp2 t0 = sub(sqr(a.c0), mul_xi(mul(a.c1, a.c2)));
    const Fp2 t1 = sub(mul_xi(sqr(a.c2)), mul(a.c0, a.c1));
    const Fp2 t2 = sub(sqr(a.c1), mul(a.c0, a.c2));
    const Fp2 d = add(mul(a.c0, t0), mul_xi(add(mul(a.c2, t1), mul(a.c1, t2))));
    const Fp2 di = inv(d);
    return {mul(t0, di), mul(t1, di), mul(t2, di)};
}
// a * (b0 + b1 v): 5 Fp2 products
PD_CALL Fp6 mul_sparse01(const Fp6 &a, const Fp2 &b0, const Fp2 &b1) {
    const Fp2 m0 = mul(a.c0, b0), m1 = mul(a.c1, b1);
    const Fp2 cross = sub(sub(mul(add(a.c0, a.c1), add(b0, b1)), m0), m1);  // a0 b1 + a1 b0
    return {add(m0, mul_xi(mul(a.c2, b1))), cross, add(m1, mul(a.c2, b0))};
}
// a * (k v) for k in Fp
HD Fp6 mul_sparse1_fp(const Fp6 &a, const Fp &k) { return {mul_xi(mul_fp(a.c2, k)), mul_fp(a.c0, k), mul_fp(a.c1, k)}; }

// ---- Fp12 ----
HD Fp12 fp12_one() {
    Fp12 r;
    r.c0.c0.c0 = Fp::one();
    r.c0.c0.c1 = Fp::zero();
    r.c0.c1 = {Fp::zero(), Fp::zero()};
    r.c0.c2 = r.c0.c1;
    r.c1.c0 = r.c0.c1;
    r.c1.c1 = r.c0.c1;
    r.c1.c2 = r.c0.c1;
    return r;
}
// an Fp12 as its 144 limbs (a copy: the limb arrays of the members are not indexed past their own 12 entries)
struct Fp12Limbs {
    uint32_t w[144];
};
static_assert(sizeof(Fp12) == sizeof(Fp12Limbs), "Fp12 is 144 limbs");
HD Fp12Limbs limbs_of(const Fp12 &f) {
    Fp12Limbs r;
    __builtin_memcpy(&r, &f, sizeof r);
    return r;
}
HD bool is_one(const Fp12 &f) {
    const Fp one = Fp::one();
    const Fp12Limbs x = limbs_of(f);
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) acc |= x.w[i] ^ one.l[i];
#pragma unroll
    for (int i = 12; i < 144; i++) acc |= x.w[i];
    return acc == 0;
}
// m ? a : b, limb by limb (m all ones or zero): no branch around the work that produced a
HD Fp12 select(uint32_t m, const Fp12 &a, const Fp12 &b) {
    const Fp12Limbs x = limbs_of(a), y = limbs_of(b);
    Fp12Limbs o;
#pragma unroll
    for (int i = 0; i < 144; i++) o.w[i] = (x.w[i] & m) | (y.w[i] & ~m);
    Fp12 r;
    __builtin_memcpy(&r, &o, sizeof r);
    return r;
}
HD Fp12 conj(const Fp12 &a) { return {a.c0, neg(a.c1)}; }
PD_CALL Fp12 mul(const Fp12 &a, const Fp12 &b) {
    const Fp6 v0 = mul(a.c0, b.c0), v1 = mul(a.c1, b.c1);
    const Fp6 c1 = sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), v0), v1);
    return {add(v0, mul_v(v1)), c1};
}
// complex squaring: 2 Fp6 products instead of 3
PD_CALL Fp12 sqr(const Fp12 &a) {
    const Fp6 v0 = mul(a.c0, a.c1);
    const Fp6 t = mul(add(a.c0, a.c1), add(a.c0, mul_v(a.c1)));
    return {sub(sub(t, v0), mul_v(v0)), add(v0, v0)};
}
// the Fp12 inverse down to ONE fp_inv: Fp12 -> Fp6 (norm over Fp6) -> Fp2 -> Fp
PD_CALL Fp12 inv(const Fp12 &a) {
    const Fp6 d = inv(sub(mul(a.c0, a.c0), mul_v(mul(a.c1, a.c1))));
    return {mul(a.c0, d), neg(mul(a.c1, d))};
}

// f * (c + (-lam*xp) v + yp v w): 2 sparse Fp6 products of 5 Fp2 products + one by an Fp multiple of v
PD_CALL Fp12 mul_by_prepared_line(const Fp12 &f, const Fp2 &lam, const Fp2 &c, const G1Affine &p) {
    const Fp2 B = neg(mul_fp(lam, p.x));
    const Fp6 t0 = mul_sparse01(f.c0, c, B);
    const Fp6 t1 = mul_sparse1_fp(f.c1, p.y);
    Fp2 By = B;
    By.c0 = add(By.c0, p.y);  // l0 + l1 = A + (B + yp) v
    const Fp6 t2 = mul_sparse01(add(f.c0, f.c1), c, By);
    return {add(t0, mul_v(t1)), sub(sub(t2, t0), t1)};
}

// The Miller-loop value of e(p1, Q1) * e(p2, Q2) with Q1, Q2 given by their line tables (MILLER_STEPS entries each).
// An infinite G1 argument makes its factor 1 (host_pairing.hpp: miller_product_prepared): here every line product is
// computed and the lane's infinity flag SELECTS whether it is kept, so that the lanes of a wave never diverge.  Every lane
// reads the same table step at the same time: the loads are wave-uniform.
HDNI inline Fp12 miller_product_tables(const G1Affine &p1, const LineTable &q1, const G1Affine &p2, const LineTable &q2) {
    const uint32_t use1 = p1.is_inf() ? 0u : ~0u, use2 = p2.is_inf() ? 0u : ~0u;
    Fp12 f = fp12_one();
    const uint64_t xabs = BLS_X_ABS;
    int n = 0;
    for (int i = 62; i >= 0; i--) {
        f = sqr(f);
        for (int rep = 0; rep < 2; rep++) {
            if (rep == 1 && !((xabs >> i) & 1)) break;   // (uniform: the addition steps of |x|)
            const LineCoeffs l1 = q1(n), l2 = q2(n);
            f = select(use1, mul_by_prepared_line(f, l1.lam, l1.c, p1), f);
            f = select(use2, mul_by_prepared_line(f, l2.lam, l2.c, p2), f);
            n++;
        }
    }
    return f;
}

// f^(p^K), K = 1..3: a_i -> conj^K(a_i) * (1+u)^(i (p^K - 1)/6) for f = sum a_i w^i (host_pairing.hpp: frobenius)
template <int K>
HD Fp2 frob_gamma(int i) {
    Fp2 g;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        g.c0.l[j] = FROB_GAMMA[K - 1][i - 1][0][j];
        g.c1.l[j] = FROB_GAMMA[K - 1][i - 1][1][j];
    }
    return g;
}
template <int K>
HDNI inline Fp12 frobenius(const Fp12 &f) {
    auto cj = [](const Fp2 &a) { return (K & 1) ? conj(a) : a; };
    Fp12 r;
    r.c0.c0 = cj(f.c0.c0);
    r.c1.c0 = mul(cj(f.c1.c0), frob_gamma<K>(1));
    r.c0.c1 = mul(cj(f.c0.c1), frob_gamma<K>(2));
    r.c1.c1 = mul(cj(f.c1.c1), frob_gamma<K>(3));
    r.c0.c2 = mul(cj(f.c0.c2), frob_gamma<K>(4));
    r.c1.c2 = mul(cj(f.c1.c2), frob_gamma<K>(5));
    return r;
}

// Granger-Scott squaring in the cyclotomic subgroup: three Fp4 squares, 9 Fp2 products instead of 18.  Valid only for
// elements of norm 1 (after the easy part of the final exponentiation).
HD void fp4_sqr(Fp2 &r0, Fp2 &r1, const Fp2 &a, const Fp2 &b) {
    const Fp2 ab = mul(a, b);
    r0 = sub(sub(mul(add(a, b), add(a, mul_xi(b))), ab), mul_xi(ab));  // a^2 + xi b^2
    r1 = dbl(ab);
}
PD_CALL Fp12 cyclotomic_sqr(const Fp12 &f) {
    const Fp2 z0 = f.c0.c0, z4 = f.c0.c1, z3 = f.c0.c2, z2 = f.c1.c0, z1 = f.c1.c1, z5 = f.c1.c2;
    Fp2 t0, t1, t2, t3, t4, t5;
    fp4_sqr(t0, t1, z0, z1);
    fp4_sqr(t2, t3, z2, z3);
    fp4_sqr(t4, t5, z4, z5);
    auto three_minus_two = [](const Fp2 &x, const Fp2 &z) { const Fp2 d = sub(x, z); return add(dbl(d), x); };  // 3x - 2z
    auto three_plus_two = [](const Fp2 &x, const Fp2 &z) { const Fp2 d = add(x, z); return add(dbl(d), x); };   // 3x + 2z
    Fp12 r;
    r.c0.c0 = three_minus_two(t0, z0);
    r.c1.c1 = three_plus_two(t1, z1);
    r.c1.c0 = three_plus_two(mul_xi(t5), z2);
    r.c0.c2 = three_minus_two(t4, z3);
    r.c0.c1 = three_minus_two(t2, z4);
    r.c1.c2 = three_plus_two(t3, z5);
    return r;
}

// g^x for the (negative) BLS parameter x, g in the cyclotomic subgroup (inverse = conjugate)
PD_CALL Fp12 pow_x(const Fp12 &g) {
    const uint64_t xabs = BLS_X_ABS;
    Fp12 acc = g;
    for (int i = 62; i >= 0; i--) {
        acc = cyclotomic_sqr(acc);
        if ((xabs >> i) & 1) acc = mul(acc, g);
    }
    return conj(acc);
}

// f^((p^12-1)/r * 3): easy part (p^6-1)(p^2+1), hard part l0 + l1 p + l2 p^2 + l3 p^3 with l3 = (x-1)^2, l2 = l3 x,
// l1 = l2 x - l3, l0 = l1 x + 3 (host_pairing.hpp: final_exp; the factor 3 is harmless for an "== 1" test)
HDNI inline Fp12 final_exp(const Fp12 &f) {
    Fp12 a = mul(conj(f), inv(f));
    a = mul(frobenius<2>(a), a);
    const Fp12 t = mul(pow_x(a), conj(a));
    const Fp12 y3 = mul(pow_x(t), conj(t));
    const Fp12 y2 = pow_x(y3);
    const Fp12 y1 = mul(pow_x(y2), conj(y3));
    const Fp12 y0 = mul(pow_x(y1), mul(cyclotomic_sqr(a), a));
    return mul(mul(y0, frobenius<1>(y1)), mul(frobenius<2>(y2), frobenius<3>(y3)));
}

// e(p1, Q1) * e(p2, Q2) == 1 ?
HDNI inline bool pairing_product_is_one(const G1Affine &p1, const LineTable &q1, const G1Affine &p2, const LineTable &q2) {
    return is_one(final_exp(miller_product_tables(p1, q1, p2, q2)));
}

}  // namespace pdev
}  // namespace ckzg
