// field_test_ops.hpp -- the arithmetic under the Fr kernels and the pairing, behind one raw-word calling convention
// (test aid, the counterpart of f28_test_ops.hpp: host_shim.cpp runs it as g++ builds it, tests/native/dev_shim_fields.hip
// as the device compiler does with the product's plain flags).  What it reaches:
//   field.hpp        Mont<FpParams> (12 words) and Mont<FrParams> (8 words): on the device the 32-bit CIOS bodies of
//                    add / sub / mul that every Fr kernel (ntt.hip, verify.hip) and the whole pairing run
//   fr29.hpp         Fr on nine 29-bit limbs, operands taken as they come (lazily reduced: limbs below 2^29, the top
//                    one holding what is left), every K / C / L instantiation the kernels of verify.hip use
//   fp28_inv.hpp, fr_inv.hpp, fr29_inv   the safegcd inversions: one update step and driver loop (fp28_inv.hpp) under
//                    three repackings (28-, 32- and 29-bit limbs)
//   tower.hpp        the tower, the Frobenius maps, the cyclotomic forms and final_exp: the ONE text of the host's and
//                    the device's pairing.  g++ with __int128 takes its lazily reduced 64-bit Fp2 product and square,
//                    the device compiler and a build with -U__SIZEOF_INT128__ the Karatsuba forms
//   pairing_dev.hpp  the two-pair Miller product against line tables the caller passes in (k_pairing_check)
// The list is the single source: every line is  X(name, WO, WA, WB, WC, WD, SHARED, statement)  -- the widths in
// 32-bit words of the result o and of the operands a, b, c, d (0: unused); SHARED = 1: c and d are the same for every
// item of a call (the line tables: lam[68] then c[68], Fp2 each, as pairing.hip lays them out).  desc() spells the
// list out for the tests, widths() for the shims.  A predicate is one word; tree_leaf is the value and then `bad`.
#pragma once
#include "fr29.hpp"
#include "pairing_dev.hpp"

#define CKZG_FT_TABLE 3264   // 2 * MILLER_STEPS Fp2 entries of 24 words

#define CKZG_FT_MONT(pf, PP, N, INV)                                                                               \
    X(pf##_mul, N, N, N, 0, 0, 0, st(o, mul(ldm<PP>(a), ldm<PP>(b))))                                              \
    X(pf##_sqr, N, N, 0, 0, 0, 0, st(o, sqr(ldm<PP>(a))))                                                          \
    X(pf##_add, N, N, N, 0, 0, 0, st(o, add(ldm<PP>(a), ldm<PP>(b))))                                              \
    X(pf##_sub, N, N, N, 0, 0, 0, st(o, sub(ldm<PP>(a), ldm<PP>(b))))                                              \
    X(pf##_neg, N, N, 0, 0, 0, 0, st(o, neg(ldm<PP>(a))))                                                          \
    X(pf##_dbl, N, N, 0, 0, 0, 0, st(o, dbl(ldm<PP>(a))))                                                          \
    X(pf##_to_raw, N, N, 0, 0, 0, 0, to_raw<PP>(o, ldm<PP>(a)))                                                    \
    X(pf##_from_raw, N, N, 0, 0, 0, 0, st(o, from_raw<PP>(a)))                                                     \
    X(pf##_inv, N, N, 0, 0, 0, 0, st(o, INV(ldm<PP>(a))))

#define CKZG_FT_SUB_BELOW(K) X(fr29_sub_below_##K, 9, 9, 9, 0, 0, 0, st(o, fr29_sub_below<K>(ld29(a), ld29(b))))
#define CKZG_FT_CANONICAL(K) X(fr29_canonical_##K, 9, 9, 0, 0, 0, 0, st(o, fr29_canonical<K>(ld29(a))))
#define CKZG_FT_COMBINE(C)                                                                                         \
    X(tree_combine_##C##_call, 9, 9, 9, 9, 0, 0, st(o, ev29::tree_combine<C, false>(ld29(a), ld29(b), ld29(c))))   \
    X(tree_combine_##C##_flat, 9, 9, 9, 9, 0, 0, st(o, ev29::tree_combine<C, true>(ld29(a), ld29(b), ld29(c))))
#define CKZG_FT_TREE_CANONICAL(L) X(tree_canonical_##L, 9, 9, 0, 0, 0, 0, st(o, ev29::tree_canonical<L>(ld29(a))))
#define CKZG_FT_FROBENIUS(K) X(frobenius_##K, 144, 144, 0, 0, 0, 0, stt(o, tower::frobenius<K>(ldt<tower::Fp12>(a))))

#define CKZG_FIELD_TEST_OPS                                                                                        \
    CKZG_FT_MONT(fp, FpParams, 12, fp_inv)                                                                         \
    CKZG_FT_MONT(fr, FrParams, 8, fr_inv)                                                                          \
    X(fr_geq_r, 1, 8, 0, 0, 0, 0, uint32_t m_[8]; mod_limbs<FrParams>(m_); st(o, limbs_geq<8>(a, m_)))             \
    X(fr29_pack, 9, 8, 0, 0, 0, 0, st(o, fr29_pack(a)))                                                            \
    X(fr29_unpack, 8, 9, 0, 0, 0, 0, fr29_unpack(o, ld29(a)))                                                      \
    X(fr29_mul, 9, 9, 9, 0, 0, 0, st(o, fr29_mul(ld29(a), ld29(b))))                                               \
    X(fr29_mul_inline, 9, 9, 9, 0, 0, 0, st(o, fr29_mul_inline(ld29(a), ld29(b))))                                 \
    X(fr29_add, 9, 9, 9, 0, 0, 0, st(o, fr29_add(ld29(a), ld29(b))))                                               \
    X(fr29_carry, 9, 9, 0, 0, 0, 0, Fr29 x_ = ld29(a); fr29_carry(x_); st(o, x_))                                  \
    CKZG_FT_SUB_BELOW(0) CKZG_FT_SUB_BELOW(2) CKZG_FT_SUB_BELOW(3) CKZG_FT_SUB_BELOW(5)                            \
    CKZG_FT_CANONICAL(0) CKZG_FT_CANONICAL(1) CKZG_FT_CANONICAL(2) CKZG_FT_CANONICAL(4) CKZG_FT_CANONICAL(5)       \
    X(fr29_equal, 1, 9, 9, 0, 0, 0, st(o, fr29_equal(ld29(a), ld29(b))))                                           \
    X(fr29_from_fr, 9, 8, 0, 0, 0, 0, st(o, fr29_from_fr(ldm<FrParams>(a))))                                       \
    X(fr29_to_fr, 8, 9, 0, 0, 0, 0, st(o, fr29_to_fr(ld29(a))))                                                    \
    X(to_fr_radix256, 8, 9, 0, 0, 0, 0, st(o, ev29::to_fr_radix256(ld29(a))))                                      \
    X(vanishing_over_n, 9, 9, 0, 0, 0, 0, st(o, ev29::vanishing_over_n(ld29(a))))                                  \
    X(scale, 8, 8, 9, 0, 0, 0, st(o, ev29::scale(ldm<FrParams>(a), ld29(b))))                                      \
    X(tree_leaf, 10, 8, 0, 0, 0, 0, uint32_t bad_ = 0; st(o, ev29::tree_leaf_from_words(a, bad_)); o[9] = bad_)    \
    CKZG_FT_COMBINE(0) CKZG_FT_COMBINE(1) CKZG_FT_COMBINE(2) CKZG_FT_COMBINE(3) CKZG_FT_COMBINE(4)                 \
    CKZG_FT_COMBINE(5)                                                                                             \
    CKZG_FT_TREE_CANONICAL(1) CKZG_FT_TREE_CANONICAL(2) CKZG_FT_TREE_CANONICAL(3) CKZG_FT_TREE_CANONICAL(4)        \
    CKZG_FT_TREE_CANONICAL(5) CKZG_FT_TREE_CANONICAL(6)                                                            \
    X(tree_finish, 8, 9, 0, 0, 0, 0, st(o, ev29::tree_finish(ld29(a))))                                            \
    X(tree_finish_from_integers, 8, 9, 0, 0, 0, 0, st(o, ev29::tree_finish_from_integers(ld29(a))))                \
    X(fr_inv_safegcd, 8, 8, 0, 0, 0, 0, st(o, fr_inv_safegcd(ldm<FrParams>(a))))                                   \
    X(fr29_inv, 9, 9, 0, 0, 0, 0, st(o, fr29_inv(ld29(a))))                                                        \
    X(f28_inv_safegcd, 14, 14, 0, 0, 0, 0, st28(o, f28_inv_safegcd(ld28(a))))                                      \
    X(fp2_mul, 24, 24, 24, 0, 0, 0, stt(o, tower::mul(ldt<tower::Fp2>(a), ldt<tower::Fp2>(b))))                    \
    X(fp2_sqr, 24, 24, 0, 0, 0, 0, stt(o, tower::sqr(ldt<tower::Fp2>(a))))                                         \
    X(fp2_inv, 24, 24, 0, 0, 0, 0, stt(o, tower::inv(ldt<tower::Fp2>(a))))                                         \
    X(fp2_mul_xi, 24, 24, 0, 0, 0, 0, stt(o, tower::mul_xi(ldt<tower::Fp2>(a))))                                   \
    X(fp2_conj, 24, 24, 0, 0, 0, 0, stt(o, tower::conj(ldt<tower::Fp2>(a))))                                       \
    X(fp2_mul_fp, 24, 24, 12, 0, 0, 0, stt(o, tower::mul_fp(ldt<tower::Fp2>(a), ldm<FpParams>(b))))                \
    X(fp6_mul, 72, 72, 72, 0, 0, 0, stt(o, tower::mul(ldt<tower::Fp6>(a), ldt<tower::Fp6>(b))))                    \
    X(fp6_inv, 72, 72, 0, 0, 0, 0, stt(o, tower::inv(ldt<tower::Fp6>(a))))                                         \
    X(fp6_mul_v, 72, 72, 0, 0, 0, 0, stt(o, tower::mul_v(ldt<tower::Fp6>(a))))                                     \
    X(fp6_mul_sparse01, 72, 72, 24, 24, 0, 0,                                                                      \
      stt(o, tower::mul_sparse01(ldt<tower::Fp6>(a), ldt<tower::Fp2>(b), ldt<tower::Fp2>(c))))                     \
    X(fp6_mul_sparse1_fp, 72, 72, 12, 0, 0, 0, stt(o, tower::mul_sparse1_fp(ldt<tower::Fp6>(a), ldm<FpParams>(b)))) \
    X(fp12_mul, 144, 144, 144, 0, 0, 0, stt(o, tower::mul(ldt<tower::Fp12>(a), ldt<tower::Fp12>(b))))              \
    X(fp12_sqr, 144, 144, 0, 0, 0, 0, stt(o, tower::sqr(ldt<tower::Fp12>(a))))                                     \
    X(fp12_inv, 144, 144, 0, 0, 0, 0, stt(o, tower::inv(ldt<tower::Fp12>(a))))                                     \
    X(fp12_conj, 144, 144, 0, 0, 0, 0, stt(o, tower::conj(ldt<tower::Fp12>(a))))                                   \
    X(fp12_select, 144, 144, 144, 1, 0, 0, stt(o, pdev::select(c[0], ldt<tower::Fp12>(a), ldt<tower::Fp12>(b))))   \
    X(fp12_is_one, 1, 144, 0, 0, 0, 0, st(o, tower::is_one(ldt<tower::Fp12>(a))))                                  \
    X(fp12_mul_by_prepared_line, 144, 144, 24, 24, 24, 0,                                                          \
      stt(o, tower::mul_by_prepared_line(ldt<tower::Fp12>(a), ldt<tower::Fp2>(b), ldt<tower::Fp2>(c), ldt<G1Affine>(d)))) \
    CKZG_FT_FROBENIUS(1) CKZG_FT_FROBENIUS(2) CKZG_FT_FROBENIUS(3)                                                 \
    X(cyclotomic_sqr, 144, 144, 0, 0, 0, 0, stt(o, tower::cyclotomic_sqr(ldt<tower::Fp12>(a))))                    \
    X(pow_x, 144, 144, 0, 0, 0, 0, stt(o, tower::pow_x(ldt<tower::Fp12>(a))))                                      \
    X(final_exp, 144, 144, 0, 0, 0, 0, stt(o, tower::final_exp(ldt<tower::Fp12>(a))))                              \
    X(miller_product_tables, 144, 24, 24, CKZG_FT_TABLE, CKZG_FT_TABLE, 1,                                         \
      stt(o, pdev::miller_product_tables(ldt<G1Affine>(a), table(c), ldt<G1Affine>(b), table(d))))                 \
    X(pairing_product_is_one, 1, 24, 24, CKZG_FT_TABLE, CKZG_FT_TABLE, 1,                                          \
      st(o, pdev::pairing_product_is_one(ldt<G1Affine>(a), table(c), ldt<G1Affine>(b), table(d))))

namespace ckzg {
namespace fieldtest {

constexpr int MAX_WORDS = 144;   // the widest result or per-item operand (an Fp12)
static_assert(CKZG_FT_TABLE == 2 * tower::MILLER_STEPS * 24, "a line table is lam[68] and c[68]");

template <class P>
HD Mont<P> ldm(const uint32_t *p) {
    Mont<P> r;
#pragma unroll
    for (int j = 0; j < P::N; j++) r.l[j] = p[j];
    return r;
}
HD Fr29 ld29(const uint32_t *p) {
    Fr29 r;
#pragma unroll
    for (int j = 0; j < 9; j++) r.l[j] = p[j];
    return r;
}
HD F28<1, 2> ld28(const uint32_t *p) {
    F28<1, 2> r;
#pragma unroll
    for (int j = 0; j < 14; j++) r.l[j] = p[j];
    return r;
}
// a tower element or an affine point: its limbs as they lie in memory
template <class T>
HD T ldt(const uint32_t *p) {
    uint32_t w[sizeof(T) / 4];
#pragma unroll
    for (size_t j = 0; j < sizeof(T) / 4; j++) w[j] = p[j];
    T r;
    __builtin_memcpy(&r, w, sizeof r);
    return r;
}
HD pdev::LineTable table(const uint32_t *p) {
    const tower::Fp2 *t = reinterpret_cast<const tower::Fp2 *>(p);
    return {t, t + tower::MILLER_STEPS};
}
template <class P>
HD void st(uint32_t *o, const Mont<P> &v) {
#pragma unroll
    for (int j = 0; j < P::N; j++) o[j] = v.l[j];
}
HD void st(uint32_t *o, const Fr29 &v) {
#pragma unroll
    for (int j = 0; j < 9; j++) o[j] = v.l[j];
}
HD void st(uint32_t *o, bool v) { o[0] = v ? 1u : 0u; }
HD void st28(uint32_t *o, const F28<1, 2> &v) {
#pragma unroll
    for (int j = 0; j < 14; j++) o[j] = v.l[j];
}
template <class T>
HD void stt(uint32_t *o, const T &v) {
    uint32_t w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof v);
#pragma unroll
    for (size_t j = 0; j < sizeof(T) / 4; j++) o[j] = w[j];
}

// operation number `op` of the list on one item: o <- op(a, b, c, d); returns false for a number past the list
HDNI inline bool run(int op, uint32_t *o, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d) {
    int n = 0;
#define X(name, WO, WA, WB, WC, WD, SH, ...) if (op == n++) { __VA_ARGS__; return true; }
    CKZG_FIELD_TEST_OPS
#undef X
    return false;
}

// w[0..4]: the widths of o, a, b, c, d in words, w[5]: c and d are shared by the items; false past the list
inline bool widths(int op, int *w) {
    int n = 0;
#define X(name, WO, WA, WB, WC, WD, SH, ...) \
    if (op == n++) { w[0] = WO; w[1] = WA; w[2] = WB; w[3] = WC; w[4] = WD; w[5] = SH; return true; }
    CKZG_FIELD_TEST_OPS
#undef X
    return false;
}

// n items on the host: operand k of item i lies at k + width * i, a shared operand at k; false past the list
inline bool run_items(int op, uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, int n) {
    int w[6];
    if (!widths(op, w)) return false;
    const size_t sc = w[5] ? 0 : w[3], sd = w[5] ? 0 : w[4];
    for (int i = 0; i < n; i++)
        if (!run(op, out + (size_t)w[0] * i, a + (size_t)w[1] * i, b + (size_t)w[2] * i, c + sc * i, d + sd * i)) return false;
    return true;
}

#define CKZG_FT_STR2(x) #x
#define CKZG_FT_STR(x) CKZG_FT_STR2(x)
// one line per operation, in order: its name, the five widths and the shared flag
inline const char *desc() {
    return ""
#define X(name, WO, WA, WB, WC, WD, SH, ...) \
    #name " " CKZG_FT_STR(WO) " " CKZG_FT_STR(WA) " " CKZG_FT_STR(WB) " " CKZG_FT_STR(WC) " " CKZG_FT_STR(WD) " " #SH "\n"
        CKZG_FIELD_TEST_OPS
#undef X
        ;
}

}  // namespace fieldtest
}  // namespace ckzg
