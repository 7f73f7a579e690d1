// tower.hpp -- the BLS12-381 pairing tower, once, for the host (host_pairing.hpp: the C-ABI's pairing checks, G2) and
// for one lane of a GPU kernel (pairing_dev.hpp, pairing.hip: k_pairing_check):
//   Fp2 = Fp[u]/(u^2+1), Fp6 = Fp2[v]/(v^3-(1+u)), Fp12 = Fp6[w]/(w^2-v),
// the sparse product by a prepared line, the Frobenius maps, the Granger-Scott square, pow_x and the final
// exponentiation (easy part with ONE fp_inv, hard part through Granger-Scott squarings and pow_x), on field.hpp's
// host/device Mont<FpParams>.  The two Miller products that walk prepared lines are not here: the host's skips an
// infinite slot (host_pairing.hpp: miller_product_prepared), the device's selects (pairing_dev.hpp).
//
// Every function has one body except the Fp2 product and square: where field.hpp takes its 64-bit host forms (a host
// pass with __int128) they are lazily reduced double-width forms -- they are why a host pairing check costs ~0.75 ms --
// and everywhere else (the device, a host build without __int128) Karatsuba over the Fp product.  Both return fully
// reduced values, so every build agrees byte for byte (tests/test_point_pairing_host.py).
//
// Code size on the device: an Fp12 is 144 VGPRs; with every product force-inlined one pairing is hundreds of thousands
// of instructions.  The Fp2 / Fp6 / Fp12 products and squares, the line product, pow_x and the inversions are therefore
// out-of-line device functions (PD_CALL); only the Fp product (field.hpp) and the cheap add / sub forms are inlined
// into them.
#pragma once
#include "g1.hpp"

// How the functions are marked.  Device pass: the large ones out of line (PD_CALL), the small ones force-inlined
// (PD_INL), as pairing_dev.hpp marked them before the tower was shared.  Every host pass, g++'s and hipcc's: both are
// plain `inline`, as host_pairing.hpp had them, and the compiler decides -- forcing the small helpers into the Fp6 /
// Fp12 products cost the host's pairing check 7 %.  (On purpose this also takes noinline off the large functions in a
// hipcc host pass, where pairing_dev.hpp had it: the host's pairing is compiled there, in ckzg_api2.hip.)
#if defined(__HIP_DEVICE_COMPILE__)
#define PD_CALL HDNI inline __attribute__((noinline))
#define PD_INL HD
#else
#define PD_CALL HDNI inline
#define PD_INL HDNI inline
#endif

namespace ckzg {
namespace tower {

constexpr int MILLER_STEPS = 68;  // 63 doublings + 5 additions for |x| = 0xd201000000010000

// Plain aggregates: the lam[] and c[] arrays of host_pairing.hpp's G2Prepared are uploaded as they lie and read by
// k_pairing_check as Fp2.
struct Fp2 {
    Fp c0, c1;
    PD_INL static Fp2 zero() { return {Fp::zero(), Fp::zero()}; }
    PD_INL static Fp2 one() { return {Fp::one(), Fp::zero()}; }
    PD_INL bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    PD_INL bool operator==(const Fp2 &o) const { return c0 == o.c0 && c1 == o.c1; }
};
struct Fp6 {
    Fp2 c0, c1, c2;
};
struct Fp12 {
    Fp6 c0, c1;
    PD_INL static Fp12 one() {
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
};
static_assert(sizeof(Fp2) == 96 && sizeof(Fp6) == 288 && sizeof(Fp12) == 576, "tower layout");

// ---- Fp2 ----
PD_INL Fp2 add(const Fp2 &a, const Fp2 &b) { return {add(a.c0, b.c0), add(a.c1, b.c1)}; }
PD_INL Fp2 sub(const Fp2 &a, const Fp2 &b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
PD_INL Fp2 neg(const Fp2 &a) { return {neg(a.c0), neg(a.c1)}; }
PD_INL Fp2 dbl(const Fp2 &a) { return add(a, a); }
PD_INL Fp2 mul_xi(const Fp2 &a) { return {sub(a.c0, a.c1), add(a.c0, a.c1)}; }  // * (1+u)
PD_INL Fp2 conj(const Fp2 &a) { return {a.c0, neg(a.c1)}; }

#if !defined(__HIP_DEVICE_COMPILE__) && defined(__SIZEOF_INT128__)
// ---- double-width helpers for lazily reduced Fp2 products (host only, 64-bit limbs) ----
struct FpWide {
    uint64_t w[12];
};
inline void fp_load64(uint64_t x[6], const Fp &a) { __builtin_memcpy(x, a.l, 48); }
// 6 x 6 -> 12 limbs, no reduction: product scanning (Comba) with a three-word column accumulator
inline void fp_mul_wide(FpWide &r, const uint64_t a[6], const uint64_t b[6]) {
    typedef unsigned __int128 u128;
    uint64_t acc0 = 0, acc1 = 0, acc2 = 0;
#pragma unroll
    for (int k = 0; k < 11; k++) {
#pragma unroll
        for (int i = (k < 6 ? 0 : k - 5); i <= (k < 6 ? k : 5); i++) {
            u128 p = (u128)a[i] * b[k - i];
            u128 s = (u128)acc0 + (uint64_t)p;
            acc0 = (uint64_t)s;
            s = (u128)acc1 + (uint64_t)(p >> 64) + (uint64_t)(s >> 64);
            acc1 = (uint64_t)s;
            acc2 += (uint64_t)(s >> 64);
        }
        r.w[k] = acc0;
        acc0 = acc1;
        acc1 = acc2;
        acc2 = 0;
    }
    r.w[11] = acc0;
}
inline void wide_add(FpWide &r, const FpWide &a, const FpWide &b) {
    typedef unsigned __int128 u128;
    u128 c = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        c += (u128)a.w[i] + b.w[i];
        r.w[i] = (uint64_t)c;
        c >>= 64;
    }
}
inline void wide_sub(FpWide &r, const FpWide &a, const FpWide &b) {  // a >= b required
    typedef unsigned __int128 u128;
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        u128 d = (u128)a.w[i] - b.w[i] - br;
        r.w[i] = (uint64_t)d;
        br = (uint64_t)(d >> 64) & 1;
    }
}
inline const FpWide &fp_p_squared() {
    static const FpWide p2 = []() {
        uint64_t m[6];
        for (int i = 0; i < 6; i++) m[i] = (uint64_t)FP_P[2 * i] | ((uint64_t)FP_P[2 * i + 1] << 32);
        FpWide r;
        fp_mul_wide(r, m, m);
        return r;
    }();
    return p2;
}
// Montgomery reduction of t < p * 2^384: t / 2^384 mod p, fully reduced
inline Fp fp_redc(const FpWide &tin) {
    typedef unsigned __int128 u128;
    uint64_t t[13], m[6];
    __builtin_memcpy(t, tin.w, sizeof tin.w);
    t[12] = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) m[i] = (uint64_t)FP_P[2 * i] | ((uint64_t)FP_P[2 * i + 1] << 32);
    constexpr uint64_t m0 = (uint64_t)FP_P[0] | ((uint64_t)FP_P[1] << 32);
    constexpr uint64_t inv32 = (uint64_t)0 - (uint64_t)FP_NINV32;
    constexpr uint64_t ninv = (uint64_t)0 - inv32 * (2 - m0 * inv32);
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const uint64_t q = t[i] * ninv;
        u128 c = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            c += (u128)q * m[j] + t[i + j];
            t[i + j] = (uint64_t)c;
            c >>= 64;
        }
#pragma unroll
        for (int k = i + 6; k < 13; k++) {
            c += t[k];
            t[k] = (uint64_t)c;
            c >>= 64;
        }
    }
    uint64_t s[6], br = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        u128 d = (u128)t[6 + i] - m[i] - br;
        s[i] = (uint64_t)d;
        br = (uint64_t)(d >> 64) & 1;
    }
    Fp r;
#pragma unroll
    for (int i = 0; i < 6; i++) s[i] = br ? t[6 + i] : s[i];
    __builtin_memcpy(r.l, s, 48);
    return r;
}
#endif

PD_CALL Fp2 mul(const Fp2 &a, const Fp2 &b) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__SIZEOF_INT128__)
    // Karatsuba with lazy reduction: three double-width products, two Montgomery reductions.
    // a0 + a1 < 2p needs no reduction (2p < 2^382), its product with b0 + b1 is < 4p^2 < p 2^384.
    typedef unsigned __int128 u128;
    uint64_t a0[6], a1[6], b0[6], b1[6], sa[6], sb[6];
    fp_load64(a0, a.c0);
    fp_load64(a1, a.c1);
    fp_load64(b0, b.c0);
    fp_load64(b1, b.c1);
    u128 ca = 0, cb = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        ca += (u128)a0[i] + a1[i];
        sa[i] = (uint64_t)ca;
        ca >>= 64;
        cb += (u128)b0[i] + b1[i];
        sb[i] = (uint64_t)cb;
        cb >>= 64;
    }
    FpWide t0, t1, t2, u;
    fp_mul_wide(t0, a0, b0);
    fp_mul_wide(t1, a1, b1);
    fp_mul_wide(t2, sa, sb);
    wide_sub(t2, t2, t0);             // a0 b1 + a1 b0 + a1 b1
    wide_sub(t2, t2, t1);             // a0 b1 + a1 b0            (< 2p^2)
    wide_add(u, t0, fp_p_squared());  // a0 b0 + p^2
    wide_sub(u, u, t1);               // a0 b0 - a1 b1 + p^2      (in (0, 2p^2))
    return {fp_redc(u), fp_redc(t2)};
#else
    // Karatsuba: 3 base-field products
    const Fp t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);
    const Fp t2 = mul(add(a.c0, a.c1), add(b.c0, b.c1));
    return {sub(t0, t1), sub(sub(t2, t0), t1)};
#endif
}
PD_CALL Fp2 sqr(const Fp2 &a) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__SIZEOF_INT128__)
    // (a0 + a1)(a0 - a1 + p) and 2 a0 a1 as double-width products: both < 4p^2 < p 2^384
    typedef unsigned __int128 u128;
    uint64_t a0[6], a1[6], s[6], d[6], m[6];
    fp_load64(a0, a.c0);
    fp_load64(a1, a.c1);
#pragma unroll
    for (int i = 0; i < 6; i++) m[i] = (uint64_t)FP_P[2 * i] | ((uint64_t)FP_P[2 * i + 1] << 32);
    u128 c = 0;
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        c += (u128)a0[i] + a1[i];
        s[i] = (uint64_t)c;
        c >>= 64;
    }
    c = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {  // a0 + p - a1 > 0
        c += (u128)a0[i] + m[i];
        uint64_t lo = (uint64_t)c;
        c >>= 64;
        u128 t = (u128)lo - a1[i] - br;
        d[i] = (uint64_t)t;
        br = (uint64_t)(t >> 64) & 1;
        // a borrow out of limb i is repaid from the carry chain's next limb via br
    }
    // the final carry and borrow cancel: a0 + p - a1 < 2p < 2^384
    FpWide t0, t1;
    fp_mul_wide(t0, s, d);
    fp_mul_wide(t1, a0, a1);
    wide_add(t1, t1, t1);
    return {fp_redc(t0), fp_redc(t1)};
#else
    const Fp m = mul(a.c0, a.c1);
    return {mul(add(a.c0, a.c1), sub(a.c0, a.c1)), dbl(m)};
#endif
}
PD_INL Fp2 mul_fp(const Fp2 &a, const Fp &k) { return {mul(a.c0, k), mul(a.c1, k)}; }
PD_CALL Fp2 inv(const Fp2 &a) {
    const Fp n = fp_inv(add(sqr(a.c0), sqr(a.c1)));
    return {mul(a.c0, n), neg(mul(a.c1, n))};
}

// ---- Fp6 ----
PD_INL Fp6 add(const Fp6 &a, const Fp6 &b) { return {add(a.c0, b.c0), add(a.c1, b.c1), add(a.c2, b.c2)}; }
PD_INL Fp6 sub(const Fp6 &a, const Fp6 &b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1), sub(a.c2, b.c2)}; }
PD_INL Fp6 neg(const Fp6 &a) { return {neg(a.c0), neg(a.c1), neg(a.c2)}; }
PD_INL Fp6 mul_v(const Fp6 &a) { return {mul_xi(a.c2), a.c0, a.c1}; }
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
PD_INL Fp6 mul_sparse1_fp(const Fp6 &a, const Fp &k) {
    return {mul_xi(mul_fp(a.c2, k)), mul_fp(a.c0, k), mul_fp(a.c1, k)};
}

// ---- Fp12 ----
// an Fp12 as its 144 limbs (a copy: the limb arrays of the members are not indexed past their own 12 entries)
struct Fp12Limbs {
    uint32_t w[144];
};
static_assert(sizeof(Fp12) == sizeof(Fp12Limbs), "Fp12 is 144 limbs");
PD_INL Fp12Limbs limbs_of(const Fp12 &f) {
    Fp12Limbs r;
    __builtin_memcpy(&r, &f, sizeof r);
    return r;
}
PD_INL bool is_one(const Fp12 &f) {
    const Fp one = Fp::one();
    const Fp12Limbs x = limbs_of(f);
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) acc |= x.w[i] ^ one.l[i];
#pragma unroll
    for (int i = 12; i < 144; i++) acc |= x.w[i];
    return acc == 0;
}
PD_INL Fp12 conj(const Fp12 &a) { return {a.c0, neg(a.c1)}; }
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

// f * (c + (-lam*xp) v + yp v w) for one step of a prepared line (slope lam, c = lam * x_T - y_T) at the G1 point p:
// l = (A + B v) + (yp v) w with A = c, B = -lam xp, and f l = (f0 l0 + v f1 l1) + (f0 l1 + f1 l0) w by Karatsuba over
// w: 2 sparse Fp6 products of 5 Fp2 products + one by an Fp multiple of v
PD_CALL Fp12 mul_by_prepared_line(const Fp12 &f, const Fp2 &lam, const Fp2 &c, const G1Affine &p) {
    const Fp2 B = neg(mul_fp(lam, p.x));
    const Fp6 t0 = mul_sparse01(f.c0, c, B);
    const Fp6 t1 = mul_sparse1_fp(f.c1, p.y);
    Fp2 By = B;
    By.c0 = add(By.c0, p.y);  // l0 + l1 = A + (B + yp) v
    const Fp6 t2 = mul_sparse01(add(f.c0, f.c1), c, By);
    return {add(t0, mul_v(t1)), sub(sub(t2, t0), t1)};
}

// f^(p^K), K = 1..3: with f = sum a_i w^i (a_i in Fp2, w^6 = 1+u), the map is
// a_i -> conj^K(a_i) * (1+u)^(i (p^K - 1)/6).  In the (c0, c1) layout a_0,a_2,a_4 are c0's and a_1,a_3,a_5 are c1's
// coefficients.
template <int K>
PD_INL Fp2 frob_gamma(int i) {
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

// Squaring in the cyclotomic subgroup (Granger-Scott): with Fp12 seen as three Fp4 = Fp2[y]/(y^2 - xi) components
// (z0,z1), (z2,z3), (z4,z5), only the three Fp4 squares are needed: 9 Fp2 products instead of 18.  Valid only for
// elements of norm 1 (after the easy part of the final exponentiation).
PD_INL void fp4_sqr(Fp2 &r0, Fp2 &r1, const Fp2 &a, const Fp2 &b) {
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

// f^((p^12-1)/r * 3).  Easy part (p^6-1)(p^2+1); hard part through
//   3 (p^4 - p^2 + 1)/r = l0 + l1 p + l2 p^2 + l3 p^3,
//   l3 = (x-1)^2, l2 = l3 x, l1 = l2 x - l3, l0 = l1 x + 3
// (identity asserted in tools/gen_constants.py).  The extra factor 3 is harmless for an "== 1" test: the result has
// order dividing r, and r is prime to 3.
HDNI inline Fp12 final_exp(const Fp12 &f) {
    Fp12 a = mul(conj(f), inv(f));          // f^(p^6-1): now unitary
    a = mul(frobenius<2>(a), a);            // ^(p^2+1): now in the cyclotomic subgroup
    const Fp12 t = mul(pow_x(a), conj(a));  // a^(x-1)
    const Fp12 y3 = mul(pow_x(t), conj(t)); // a^((x-1)^2)
    const Fp12 y2 = pow_x(y3);
    const Fp12 y1 = mul(pow_x(y2), conj(y3));
    const Fp12 y0 = mul(pow_x(y1), mul(cyclotomic_sqr(a), a));
    return mul(mul(y0, frobenius<1>(y1)), mul(frobenius<2>(y2), frobenius<3>(y3)));
}

}  // namespace tower
}  // namespace ckzg
