// fp30.hpp -- Fp on 13 SIGNED limbs of 30 bits, Montgomery radix 2^390: the field layer of the throughput
// accumulate loop (g1_30.hpp, msm.hip: msm_sum_pairs30).  Everything else keeps the 14 x 28-bit form of fp28.hpp.
//
// Why: the accumulate kernel is bound by the issue of its multiply-adds, and a column-wise product on 13 limbs
// needs 13*13 + 13*13 = 338 of them where 14 limbs need 392 (square 260 / 301, fused two-product 507 / 588).
// A 30-bit limb leaves an UNSIGNED 64-bit column no room (26 terms of 2^60), a signed one does: with balanced limbs,
// |limb| <= 2^29, a term is at most 2^58 in magnitude and 26 of them plus the carry stay below 2^63.  On gfx950
// v_mad_i64_i32 and v_ashrrev_i64 issue at the rates of v_mad_u64_u32 and v_lshrrev_b64 (tools/ubench/instr_rates.hip,
// profiles/HISTORY.md).
//
// F30<LB, VB>: every limb is at most LB * 2^29 in magnitude and the value is at most VB * p in magnitude.  A value
// may be negative; it stands for its residue mod p.  "Normalised" is LB = 1.  Signed limbs need no +k*p offsets in a
// subtraction, but the column has no headroom for lazy limbs either: EVERY product operand is normalised
// (static_assert), so sums and differences go through norm() before they are multiplied.
//
// Montgomery product, column-wise on one signed accumulator: column k receives its a_i*b_(k-i) and q_i*p_(k-i)
// terms; the first 13 columns fix their quotient digit q_k = sign-extended low 30 bits of -column/p, which makes the
// column divisible by 2^30, and an arithmetic shift carries it into the next one.  The digits are balanced as well,
// |q| <= 2^389 (1 + 2^-29), so   |a*b/2^390 mod p| <= |a*b| / 2^390 + p/2 (1 + 2^-29):
// with |a| <= VA p, |b| <= VB p and 2^390 / p > 629 a product of VA*VB <= 314 comes out at most p in magnitude.
// Its limbs 0..11 are balanced 30-bit digits, in [-2^29, 2^29); limb 12 is what is left of a value of at most
// p < 2^381: normalised.
#pragma once
#include "fp28.hpp"

namespace ckzg {

#include "fp30_consts.inc"

template <int LB, int VB>
struct F30 {
    int32_t l[13];
};

// low 30 bits, sign-extended: one v_bfe_i32
HD int32_t f30_sext(uint32_t v) { return (int32_t)(v << 2) >> 2; }

HD void mad64s(int64_t &acc, int32_t a, int32_t b) { acc += (int64_t)a * b; }

// A result column k = 13..24: take its balanced digit d in [-2^29, 2^29) and carry (acc - d) / 2^30 on.  A plain
// arithmetic shift would carry the floor, one short whenever d < 0; the accumulator is biased by 2^29 instead, which
// makes the digit (low 30 bits) - 2^29 and the shift exact.  The bias of two columns, 2^29 + 2^59, goes in at every
// second one, so it costs half a 64-bit addition per column; 2^59 counts as two terms of the column's budget.
HD int32_t f30_take_digit(int64_t &acc, int k) {
    if ((k & 1) != 0) acc += ((int64_t)1 << 29) + ((int64_t)1 << 59);
    const int32_t d = (int32_t)((uint32_t)acc & 0x3fffffffu) - (1 << 29);
    acc >>= 30;
    return d;
}

#if defined(__HIP_DEVICE_COMPILE__) && defined(CKZG_F28_ASM_BLOCKS)
#define CKZG_F30_USE_ASM_BLOCKS 1
#include "fp30_asm_cols.inc"
#endif

namespace f30detail {
// terms of magnitude <= 2^58 that a signed 64-bit column takes next to a carry-in (< 2^34): 31 * 2^58 + 2^34 < 2^63
constexpr int MAX_TERMS = 31;
}  // namespace f30detail

template <int VA, int VB>
HD F30<1, 1> mul(const F30<1, VA> &a, const F30<1, VB> &b) {
    static_assert(13 + 13 + 2 <= f30detail::MAX_TERMS, "signed 64-bit column accumulator would overflow");
    static_assert(VA * VB <= 314, "Montgomery product would exceed p in magnitude");
#ifdef CKZG_F30_USE_ASM_BLOCKS
    {
        F30<1, 1> ra;
        f30asm_mul(ra.l, a.l, b.l);
        return ra;
    }
#endif
    int32_t q[13];
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 13; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) mad64s(acc, a.l[i], b.l[k - i]);
#pragma unroll
        for (int i = 0; i < k; i++) mad64s(acc, q[i], F30_P[k - i]);
        q[k] = f30_sext((uint32_t)acc * F30_NINV);
        mad64s(acc, q[k], F30_P[0]);
        acc >>= 30;
    }
    F30<1, 1> r;
#pragma unroll
    for (int k = 13; k < 25; k++) {
#pragma unroll
        for (int i = k - 12; i < 13; i++) mad64s(acc, a.l[i], b.l[k - i]);
#pragma unroll
        for (int i = k - 12; i < 13; i++) mad64s(acc, q[i], F30_P[k - i]);
        r.l[k - 13] = f30_take_digit(acc, k);
    }
    r.l[12] = (int32_t)acc;
    return r;
}

// (a*b + c*d)/2^390 mod p with ONE reduction: 507 multiply-adds instead of 676.  Columns F30_SPLIT_LO..HI hold
// 33 to 39 terms, more than the accumulator takes: there the a*b + c*d part (at most 26 terms) is carried out
// first -- its upper part set aside, its low 30 bits left in -- and the q*p part (at most 13 terms) added after it.
template <int VA, int VB, int VC, int VD>
HD F30<1, 1> mul_add2(const F30<1, VA> &a, const F30<1, VB> &b, const F30<1, VC> &c, const F30<1, VD> &d) {
    static_assert(3 * (F30_SPLIT_LO - 1 + 1) <= f30detail::MAX_TERMS && 3 * (25 - (F30_SPLIT_HI + 1)) <= f30detail::MAX_TERMS,
                  "an unsplit column would overflow");
    static_assert(13 + 13 <= f30detail::MAX_TERMS && 1 + 13 + 2 <= f30detail::MAX_TERMS, "a split column would overflow");
    static_assert(VA * VB + VC * VD <= 314, "Montgomery result would exceed p in magnitude");
#ifdef CKZG_F30_USE_ASM_BLOCKS
    {
        F30<1, 1> ra;
        f30asm_mul_add2(ra.l, a.l, b.l, c.l, d.l);
        return ra;
    }
#endif
    int32_t q[13];
    int64_t acc = 0;
    F30<1, 1> r;
#pragma unroll
    for (int k = 0; k < 25; k++) {
        const int lo = k < 13 ? 0 : k - 12, hi = k < 13 ? k : 12;
#pragma unroll
        for (int i = lo; i <= hi; i++) mad64s(acc, a.l[i], b.l[k - i]);
#pragma unroll
        for (int i = lo; i <= hi; i++) mad64s(acc, c.l[i], d.l[k - i]);
        int64_t up = 0;
        if (k >= F30_SPLIT_LO && k <= F30_SPLIT_HI) {
            up = acc >> 30;
            acc &= 0x3fffffff;
        }
#pragma unroll
        for (int i = lo; i <= hi; i++)
            if (k - i >= 1) mad64s(acc, q[i], F30_P[k - i]);
        if (k < 13) {
            q[k] = f30_sext((uint32_t)acc * F30_NINV);
            mad64s(acc, q[k], F30_P[0]);
            acc >>= 30;
        } else {
            r.l[k - 13] = f30_take_digit(acc, k);
        }
        acc += up;
    }
    r.l[12] = (int32_t)acc;
    return r;
}

// Montgomery square: the 78 cross products are taken once against a doubled operand: 260 multiply-adds.
template <int VA>
HD F30<1, 1> sqr(const F30<1, VA> &a) {
    // column k holds at most 6 doubled cross terms (2^59 each: twelve units) + one square + 13 q*p terms
    static_assert(12 + 1 + 13 + 2 <= f30detail::MAX_TERMS, "signed 64-bit column accumulator would overflow");
    static_assert(VA * VA <= 314, "Montgomery product would exceed p in magnitude");
    int32_t d[13], q[13];
#pragma unroll
    for (int j = 0; j < 13; j++) d[j] = a.l[j] * 2;   // |d| <= 2^30
#ifdef CKZG_F30_USE_ASM_BLOCKS
    {
        F30<1, 1> ra;
        f30asm_sqr(ra.l, a.l, d);
        return ra;
    }
#endif
    int64_t acc = 0;
    F30<1, 1> r;
#pragma unroll
    for (int k = 0; k < 25; k++) {
        const int lo = k < 13 ? 0 : k - 12, hi = k < 13 ? k : 12;
#pragma unroll
        for (int i = lo; 2 * i < k; i++) mad64s(acc, a.l[i], d[k - i]);
        if ((k & 1) == 0) mad64s(acc, a.l[k / 2], a.l[k / 2]);
#pragma unroll
        for (int i = lo; i <= hi; i++)
            if (k - i >= 1) mad64s(acc, q[i], F30_P[k - i]);
        if (k < 13) {
            q[k] = f30_sext((uint32_t)acc * F30_NINV);
            mad64s(acc, q[k], F30_P[0]);
            acc >>= 30;
        } else {
            r.l[k - 13] = f30_take_digit(acc, k);
        }
    }
    r.l[12] = (int32_t)acc;
    return r;
}

template <int LA, int VA, int LB, int VB>
HD F30<LA + LB, VA + VB> add(const F30<LA, VA> &a, const F30<LB, VB> &b) {
    static_assert(LA + LB <= 3, "limb would overflow 32 bits");
    F30<LA + LB, VA + VB> r;
#pragma unroll
    for (int j = 0; j < 13; j++) r.l[j] = a.l[j] + b.l[j];
    return r;
}

template <int LA, int VA, int LB, int VB>
HD F30<LA + LB, VA + VB> sub(const F30<LA, VA> &a, const F30<LB, VB> &b) {
    static_assert(LA + LB <= 3, "limb would overflow 32 bits");
    F30<LA + LB, VA + VB> r;
#pragma unroll
    for (int j = 0; j < 13; j++) r.l[j] = a.l[j] - b.l[j];
    return r;
}

// carry-propagate to balanced limbs: limbs 0..11 in [-2^29, 2^29), limb 12 takes what the value leaves
// (|value| <= VA p < VA 2^381: at most VA 2^21 + 1)
template <int LA, int VA>
HD F30<1, VA> norm(const F30<LA, VA> &a) {
    static_assert(LA <= 3, "limb plus carry would overflow 32 bits");
    static_assert(VA <= 200, "top limb bound");
    F30<1, VA> r;
    int32_t c = 0;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        const int32_t v = a.l[j] + c;         // |v| <= LA * 2^29 + 2
        r.l[j] = f30_sext((uint32_t)v);
        // (v - digit) / 2^30; at LA = 3 the difference itself could reach 2^31, so take it from the two shifts
        c = LA <= 2 ? (v - r.l[j]) >> 30 : (v >> 30) - (r.l[j] >> 31);
    }
    r.l[12] = a.l[12] + c;
    return r;
}

template <int V>
HD F30<1, V> f30_neg(const F30<1, V> &a) {
    F30<1, V> r;
#pragma unroll
    for (int j = 0; j < 13; j++) r.l[j] = -a.l[j];
    return r;
}

template <int V>
HD F30<1, V> f30_const(const int32_t (&c)[13]) {
    F30<1, V> r;
#pragma unroll
    for (int j = 0; j < 13; j++) r.l[j] = c[j];
    return r;
}

// 12 packed 32-bit words (an integer < p) -> 13 balanced limbs, with no carry chain: a 30-bit field f_j becomes
// sext30(f_j) + (bit 29 of f_(j-1)), which is in [-2^29, 2^29]; the top field is below 2^21 and sends nothing up.
HD F30<1, 1> f30_unpack(const uint32_t *w) {
    F30<1, 1> r;
    uint32_t f[13];
#pragma unroll
    for (int j = 0; j < 13; j++) {
        const int bit = 30 * j, k = bit >> 5, sh = bit & 31;
        uint32_t lo = w[k] >> sh;
        if (sh > 2 && k + 1 < 12) lo |= w[k + 1] << (32 - sh);
        f[j] = lo;
    }
#pragma unroll
    for (int j = 0; j < 13; j++) {
        const int32_t s = j < 12 ? f30_sext(f[j]) : (int32_t)f[j];
        r.l[j] = j == 0 ? s : s + (int32_t)((f[j - 1] >> 29) & 1u);
    }
    return r;
}

// A value of at most p in magnitude, as a product leaves it -> the 14 x 28-bit form, in [0, 2p]: add p, carry
// into unsigned 30-bit fields, cut those into 28-bit ones.
HD F28<1, 2> f30_to_f28(const F30<1, 1> &a) {
    uint32_t f[13];
    int32_t c = 0;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        const int32_t v = a.l[j] + F30_P[j] + c;
        f[j] = (uint32_t)v & 0x3fffffffu;
        c = v >> 30;
    }
    f[12] = (uint32_t)(a.l[12] + F30_P[12] + c);   // the value is >= 0: so is its top field
    F28<1, 2> r;
#pragma unroll
    for (int j = 0; j < 14; j++) {
        const int bit = 28 * j, k = bit / 30, sh = bit - 30 * k;
        uint32_t lo = f[k] >> sh;
        if (sh > 2 && k + 1 < 13) lo |= f[k + 1] << (30 - sh);
        r.l[j] = j == 13 ? lo : (lo & M28);
    }
    return r;
}

}  // namespace ckzg
