// dev_shim.hip -- the device-only arithmetic behind a C ABI, the counterpart of csrc/host_shim.cpp for what g++
// never sees: the F28 product as the DEVICE compiler builds it, its inline-asm form (CKZG_F28_ASM_BLOCKS), all of
// g1_quad.hpp (the DPP-quad group law), the straight-line routines of g1_pipe.hpp (xyzz28_addsub_quad,
// jac28_add_quad_pipe, naf2_128, naf_masks), f28_inv_safegcd, g1.hpp's complete xyzz_add / xyzz_dbl on 32-bit limbs, and
// the accumulate loop's own arithmetic: Fp on 13 signed 30-bit limbs (fp30.hpp, in the asm build its generated products)
// and the mixed addition on it (g1_30.hpp), through f30_test_ops.hpp (tests/test_gpu_fp30.py).
// The fields under the Fr kernels and the pairing are in dev_shim_fields.hip (one plain build, ds_dev_*).  Test aid only
// (tests/test_gpu_dev_arith.py); never part of libckzg_hip.so.
//
// ONE source, compiled twice: with the product's plain flags and -D'DS(x)=ds_plain_##x', and with
// -DCKZG_F28_ASM_BLOCKS -D'DS(x)=ds_asm_##x'.  Both objects link into libdev_shim.so (c-kzg-4844_amd/Makefile).
//
// Every exported function takes host pointers, allocates, copies, launches ONE kernel on a stream of its own, waits
// with a deadline (polls hipStreamQuery, gives up after ~20 s with DS_DEADLINE: no unbounded synchronise), copies
// back, frees and returns the HIP error code (0 = ok).  Kernels hold bounded loops only; the LDS-spinning
// pipeline waves of g1_pipe.hpp (pipe_doubler / pipe_adder / pipe_wait) are deliberately not here.
//
// Conventions.  Field: 14 uint32 limbs per operand in and out, taken as they come (f28_test_ops.hpp); the 30-bit field:
// 13 int32 limbs per operand, 14 words per result, an accumulator as 52 int32 and two flag bytes (f30_test_ops.hpp).  Points:
// G1Jac (144 bytes, 2^384 domain, Z = 0 for infinity) in and out; an affine point travels as a G1Jac with Z = 1.
// Conversion to XYZZ28 / JAC28 / JACT28 happens in the kernel with the helpers the product kernels use.
// Geometry.  `block` threads per workgroup (a multiple of 64, at most 256).  The point kernels give every item a DPP quad (four
// lanes) and write the result of EACH of the four lanes: out[4 * item + lane].  Quads past the last item of the
// last workgroup repeat the last item and write nothing -- the product never runs a partly filled quad either (a DPP
// read of an inactive lane returns 0): its quad kernels pad the same way (fk20.hip k_g1_fft_twiddle_quad,
// verify.hip k_subgroup_g1_quad).  One-lane routines run in all four lanes of the quad on the same input.
#include "dev_shim_common.hpp"
#include "f28_test_ops.hpp"
#include "f30_test_ops.hpp"
#include "g1_pipe.hpp"
#include "dev_inline.hpp"

#ifndef DS
#error "compile with -D'DS(x)=ds_plain_##x' or -D'DS(x)=ds_asm_##x'"
#endif

using namespace ckzg;

namespace {

// ---- in-kernel conversions ----
__device__ __forceinline__ F28<1, 1> table_coord(const Fp &v) {   // the stored form of a table coordinate (msm.hip)
    Fp k8;
    for (int i = 0; i < 12; i++) k8.l[i] = FP_MONT_2POW8[i];
    const Fp t = mul(v, k8);
    return f28_unpack<1>(t.l);
}
__device__ __forceinline__ Fp table_words(const Fp &v) {   // the same coordinate as the kernel gathers it: 12 packed words
    Fp k8;
    for (int i = 0; i < 12; i++) k8.l[i] = FP_MONT_2POW8[i];
    return mul(v, k8);
}
__device__ __forceinline__ XYZZ28 load_xyzz(const G1Jac &p, bool &inf) { return xyzz28_from_xyzz(xyzz_from_jac(p), inf); }
__device__ __forceinline__ G1Jac store_xyzz(const XYZZ28 &v, bool inf) { return jac_from_xyzz(xyzz28_to_xyzz(v, inf)); }
__device__ __forceinline__ G1Jac store_jac(const JAC28 &v, bool inf) {
    if (inf) return G1Jac::inf();
    return store_xyzz(jac28_to_xyzz(v), false);
}
__device__ __forceinline__ F28<1, 2> zero12() {
    F28<1, 2> z;
#pragma unroll
    for (int j = 0; j < 14; j++) z.l[j] = 0;
    return z;
}

// item and quad lane of this thread; false for the padding quads (which then work on the last item)
__device__ __forceinline__ bool quad_item(int n, int &item, int &ql) {
    const size_t q = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 2;
    ql = (int)(threadIdx.x & 3);
    const bool live = q < (size_t)n;
    item = live ? (int)q : n - 1;
    return live;
}

}  // namespace

// ---- field: one thread per item ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_field)(int op, uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, int n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    uint32_t o[14];
    if (!f28test::run(op, o, a + 14 * i, b + 14 * i, c + 14 * i, d + 14 * i)) return;
    for (int j = 0; j < 14; j++) out[14 * i + j] = o[j];
}

// ---- f28_inv_safegcd (fp28_inv.hpp; it ends in an F28 product, so it exists in both forms): one thread per item, 14
// limbs in and out; lanes past n repeat the last item and store nothing ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_f28_inv)(uint32_t *out, const uint32_t *a, int n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const bool live = i < (size_t)n;
    if (!live) i = (size_t)n - 1;
    F28<1, 2> x;
    for (int j = 0; j < 14; j++) x.l[j] = a[14 * i + j];
    const F28<1, 2> y = f28_inv_safegcd(x);
    if (live)
        for (int j = 0; j < 14; j++) out[14 * i + j] = y.l[j];
}

// ---- additions.  kind: 0 xyzz28_add  1 jac28_add  2 xyzz28_madd (b affine)  3 jac28_add_quad  4 jac28_add_quad_zz
// 5 jac28_madd_quad_zz (b affine)  6 jac28_add_quad_pipe  7 xyzz28_add_quad  8 xyzz28_addsub_quad
// 9 xyzz_add (g1.hpp, 32-bit limbs: what k_point_lhs sums its ladder results with).
// flags bit 0: add -b.  zzok (kinds 4..6): the carried square equals Z^2 of the result. ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_add)(int kind, G1Jac *out, uint8_t *zzok, const G1Jac *a, const G1Jac *b, const uint8_t *flags, int n) {
    int item, ql;
    const bool live = quad_item(n, item, ql);
    const G1Jac pa = a[item], pb = b[item];
    const bool neg = (flags[item] & 1) != 0;
    bool ai, bi;
    XYZZ28 xa = load_xyzz(pa, ai), xb = load_xyzz(pb, bi);
    G1Jac r = G1Jac::inf();
    uint8_t ok = 1;
    if (kind == 0 || kind == 7 || kind == 8) {
        if (kind == 0) xyzz28_add(xa, ai, neg ? xyzz28_neg(xb) : xb, bi);
        else if (kind == 7) quad::xyzz28_add_quad(xa, ai, neg ? xyzz28_neg(xb) : xb, bi, ql);
        else quad::xyzz28_addsub_quad(xa, ai, xb, bi, neg, ql);
        r = store_xyzz(xa, ai);
    } else if (kind == 9) {
        const G1XYZZ ga = xyzz_from_jac(pa), gb = xyzz_from_jac(pb);
        r = jac_from_xyzz(xyzz_add(ga, neg ? xyzz_neg(gb) : gb));
    } else if (kind == 2) {
        if (!bi) xyzz28_madd(xa, ai, table_coord(pb.x), cneg_reduced(table_coord(pb.y), neg));
        r = store_xyzz(xa, ai);
    } else if (!bi) {   // the Jacobian forms take a finite second operand
        JAC28 ja;
        F28<1, 2> zz = zero12();
        if (!ai) {
            ja = jac28_from_xyzz(xa);
            zz = sqr(ja.z);
        }
        const JAC28 jb = jac28_from_xyzz(xb);
        JACT28 tb = jac28_table_entry(jb);
        if (kind == 1 || kind == 3 || kind == 4) {
            if (neg) tb = jact28_neg(tb);
            if (kind == 1) jac28_add(ja, ai, tb);
            else if (kind == 3) quad::jac28_add_quad(ja, ai, tb, ql);
            else quad::jac28_add_quad_zz(ja, zz, ai, tb, ql);
        } else if (kind == 5) {
            // the affine point on the curve the accumulator lives on (here the curve itself: Zc = 1)
            quad::jac28_madd_quad_zz(ja, zz, ai, widen<1, 20>(f28_from_fp(pb.x)), widen<1, 20>(f28_from_fp(pb.y)), neg, ql);
        } else if (kind == 6) {
            quad::jac28_add_quad_pipe(ja, zz, ai, jb.x, jb.y, jb.z, tb.zz, neg, ql);
        }
        if (kind >= 4 && !ai) ok = f28_equal(zz, sqr(ja.z)) ? 1 : 0;
        r = store_jac(ja, ai);
    }
    if (live) {
        out[4 * (size_t)item + ql] = r;
        zzok[4 * (size_t)item + ql] = ok;
    }
}

// ---- doubling chains.  kind: 0 jac28_dbl  1 jac28_dbl_quad  2 jac28_dbl_quad_zz  3 xyzz_dbl (g1.hpp, 32-bit limbs);
// steps[i] doublings of a[i] ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_dbl)(int kind, G1Jac *out, uint8_t *zzok, const G1Jac *a, const uint32_t *steps, int n) {
    int item, ql;
    const bool live = quad_item(n, item, ql);
    bool ai;
    const XYZZ28 xa = load_xyzz(a[item], ai);
    JAC28 ja = jac28_from_xyzz(xa);
    F28<1, 2> zz = sqr(ja.z);
    const int ns = (int)(steps[item] < (uint32_t)MAX_CHAIN ? steps[item] : (uint32_t)MAX_CHAIN);
    uint8_t ok = 1;
    G1XYZZ ga = xyzz_from_jac(a[item]);
    for (int s = 0; s < ns; s++) {
        if (kind == 3) ga = xyzz_dbl(ga);
        else if (kind == 0) jac28_dbl(ja);
        else if (kind == 1) quad::jac28_dbl_quad(ja, ql);
        else {
            quad::jac28_dbl_quad_zz(ja, zz, ql);
            if (!f28_equal(zz, sqr(ja.z))) ok = 0;
        }
    }
    if (live) {
        out[4 * (size_t)item + ql] = kind == 3 ? jac_from_xyzz(ga) : store_jac(ja, ai);
        zzok[4 * (size_t)item + ql] = ok;
    }
}

// ---- scalar multiplications.  kind: 0 xyzz28_mul_w4 (255-bit k)  1 xyzz28_mul_glv_w4  2 xyzz28_mul_glv_naf
// 3 xyzz28_mul_w4_128 (k words 0..3)  4 xyzz28_mul_w4_128_quad  5 xyzz28_mul_glv_naf_quad.  k: 8 words per item;
// halves != 0 (kinds 1, 2, 5): words 0..3 and 4..7 ARE the two halves k1, k2, else they come from glv_split(k). ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_mul)(int kind, G1Jac *out, const G1Jac *p, const uint32_t *k, int halves, int n) {
    int item, ql;
    const bool live = quad_item(n, item, ql);
    bool pi, oi = true;
    const XYZZ28 xp = load_xyzz(p[item], pi);
    XYZZ28 o;
    uint32_t kk[8], glv[8];
    for (int j = 0; j < 8; j++) kk[j] = glv[j] = k[8 * (size_t)item + j];
    if (!halves) glv_split(kk, glv, glv + 4);
    if (kind == 0) xyzz28_mul_w4(o, oi, xp, pi, kk);
    else if (kind == 1) xyzz28_mul_glv_w4(o, oi, xp, pi, glv);
    else if (kind == 3) xyzz28_mul_w4_128(o, oi, xp, pi, kk);
    else if (kind == 4) quad::xyzz28_mul_w4_128_quad(o, oi, xp, pi, kk, ql);
    else if (kind == 2 || kind == 5) {
        int8_t naf[2 * GLV_NAF_LEN];
        wnaf4_128(naf, glv);
        wnaf4_128(naf + GLV_NAF_LEN, glv + 4);
        if (kind == 2) xyzz28_mul_glv_naf(o, oi, xp, pi, naf, naf + GLV_NAF_LEN);
        else quad::xyzz28_mul_glv_naf_quad(o, oi, xp, pi, naf, naf + GLV_NAF_LEN, ql);
    }
    if (live) out[4 * (size_t)item + ql] = store_xyzz(o, oi);
}

// ---- subgroup test and [|x|]P of finite curve points (Z = 1).  kind: 0 g1_28_in_subgroup  1 g1_28_in_subgroup_quad
// 2 jac28_mul_bls_x_quad  3 jac28_mul_bls_x.  verdict: 1 in the subgroup / 0 not (kinds 0, 1); out: the multiple (2, 3) ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_subgroup)(int kind, G1Jac *out, uint8_t *verdict, const G1Jac *p, int n) {
    int item, ql;
    const bool live = quad_item(n, item, ql);
    const G1Jac pp = p[item];
    const F28<1, 2> x = f28_from_fp(pp.x), y = f28_from_fp(pp.y);
    G1Jac r = G1Jac::inf();
    uint8_t v = 0;
    if (kind == 0) v = g1_28_in_subgroup(x, y) ? 1 : 0;
    else if (kind == 1) v = quad::g1_28_in_subgroup_quad(x, y, ql) ? 1 : 0;
    else {
        JAC28 j, q;
        j.x = widen<1, 34>(x);
        j.y = widen<1, 34>(y);
        j.z = widen<2, 4>(f28_one());
        bool qi;
        if (kind == 2) quad::jac28_mul_bls_x_quad(q, qi, j, false, ql);
        else jac28_mul_bls_x(q, qi, j, false);
        r = store_jac(q, qi);
    }
    if (live) {
        out[4 * (size_t)item + ql] = r;
        verdict[4 * (size_t)item + ql] = v;
    }
}

// ---- chains of mixed additions, one thread per chain.  kind: 0 xyzz28_madd (sign through cneg_reduced)
// 1 xyzz28_madd_alt + xyzz28_fix_sign.  Chain c adds pts[start[c] .. start[c + 1]) (affine, Z = 1). ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_chain)(int kind, G1Jac *out, const G1Jac *pts, const uint8_t *signs, const uint32_t *start, int n) {
    const size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (c >= (size_t)n) return;
    XYZZ28 acc;
    bool inf = true, yneg = false;
    const uint32_t b = start[c];
    const int len = (int)(start[c + 1] - b < (uint32_t)MAX_CHAIN ? start[c + 1] - b : (uint32_t)MAX_CHAIN);
    for (int i = 0; i < len; i++) {
        const G1Jac pt = pts[b + i];
        const bool sg = signs[b + i] != 0;
        if (kind == 0) xyzz28_madd(acc, inf, table_coord(pt.x), cneg_reduced(table_coord(pt.y), sg));
        else xyzz28_madd_alt(acc, inf, yneg, table_coord(pt.x), table_coord(pt.y), sg);
    }
    if (kind == 1) xyzz28_fix_sign(acc, inf, yneg);
    out[c] = store_xyzz(acc, inf);
}

// ---- Fp on 13 signed 30-bit limbs (fp30.hpp; f30_test_ops.hpp): one thread per item, 13 int32 per operand, 14 words out ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_f30field)(int op, int32_t *out, const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    int32_t o[14];
    if (!f30test::run(op, o, a + 13 * i, b + 13 * i, c + 13 * i, d + 13 * i)) return;
    for (int j = 0; j < 14; j++) out[14 * i + j] = o[j];
}

// ---- the accumulate loop's mixed addition on raw state (g1_30.hpp; f30_test_ops.hpp), one thread per item.
// kind: 0 xyzz30_madd_alt (flags in: inf, yneg, dneg; out: inf, yneg)  1 xyzz30_apply_phi
// 2 xyzz30_to_xyzz28 + xyzz30_met_equal_x (56 words and the verdict in oflags) ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_step30)(int kind, int32_t *out, uint8_t *oflags, const int32_t *state, const uint8_t *flags, const uint32_t *entry, int n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    const int32_t *s = state + f30test::STATE_WORDS * i;
    if (kind == 0) {
        int32_t o[f30test::STATE_WORDS];
        uint8_t of[2];
        uint8_t f[3] = {flags[3 * i], flags[3 * i + 1], flags[3 * i + 2]};
        uint32_t e[f30test::ENTRY_WORDS];
        for (int j = 0; j < f30test::ENTRY_WORDS; j++) e[j] = entry[f30test::ENTRY_WORDS * i + j];
        f30test::madd_step(o, of, s, f, e);
        for (int j = 0; j < f30test::STATE_WORDS; j++) out[f30test::STATE_WORDS * i + j] = o[j];
        oflags[2 * i] = of[0];
        oflags[2 * i + 1] = of[1];
    } else if (kind == 1) {
        int32_t o[f30test::STATE_WORDS];
        f30test::phi_step(o, s);
        for (int j = 0; j < f30test::STATE_WORDS; j++) out[f30test::STATE_WORDS * i + j] = o[j];
    } else {
        uint32_t o[f30test::EXIT_WORDS];
        uint8_t met;
        f30test::exit_step(o, &met, s);
        for (int j = 0; j < f30test::EXIT_WORDS; j++) out[f30test::EXIT_WORDS * i + j] = (int32_t)o[j];
        oflags[i] = met;
    }
}

// ---- one lane's chain of the accumulate loop, one thread per chain (host_shim.cpp: hs_g1_madd_alt_chain_form has the
// same semantics).  Chain c takes pts[start[c] .. start[c + 1]) (affine, Z = 1), skipped where at_inf, negated where
// signs, phi applied before its entry phi_at[c] (at the end if the chain is shorter).  form 0: the 28-bit law;
// 1: the 30-bit law through entry and exit; 2: the 30-bit law, and the 28-bit one again if the exit finds ZZ = 0.
// met: the exit's equal-x verdict (form 0: 0). ----
__device__ __forceinline__ void chain28(XYZZ28 &acc, bool &inf, bool &yneg, const G1Jac *pts, const uint8_t *signs, const uint8_t *at_inf, int len, uint32_t phi_at) {
    inf = true, yneg = false;
    bool phi_pending = true;
    for (int i = 0; i < len; i++) {
        if (phi_pending && (uint32_t)i >= phi_at) {
            if (!inf) acc.x = widen<1, 10>(mul(acc.x, f28_const<1, 1>(FP28_BETA_LAMBDA)));
            phi_pending = false;
        }
        if (at_inf[i]) continue;
        const G1Jac pt = pts[i];
        xyzz28_madd_alt(acc, inf, yneg, table_coord(pt.x), table_coord(pt.y), signs[i] != 0);
    }
    if (phi_pending && !inf) acc.x = widen<1, 10>(mul(acc.x, f28_const<1, 1>(FP28_BETA_LAMBDA)));
}

__global__ __launch_bounds__(MAX_BLOCK) void DS(k_chain30)(int form, G1Jac *out, uint8_t *met_out, const G1Jac *pts, const uint8_t *signs, const uint8_t *at_inf, const uint32_t *start, const uint32_t *phi_at, int n) {
    const size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (c >= (size_t)n) return;
    const uint32_t b = start[c];
    const int len = (int)(start[c + 1] - b < (uint32_t)MAX_CHAIN ? start[c + 1] - b : (uint32_t)MAX_CHAIN);
    const uint32_t phi = phi_at[c];
    XYZZ28 acc28;
    bool inf = true, yneg = false;
    uint8_t met = 0;
    if (form == 0) {
        chain28(acc28, inf, yneg, pts + b, signs + b, at_inf + b, len, phi);
    } else {
        XYZZ30 acc;
        bool phi_pending = true;
        for (int i = 0; i < len; i++) {
            if (phi_pending && (uint32_t)i >= phi) {
                if (!inf) xyzz30_apply_phi(acc);
                phi_pending = false;
            }
            if (at_inf[b + i]) continue;
            const G1Jac pt = pts[b + i];
            const Fp x = table_words(pt.x), y = table_words(pt.y);
            xyzz30_madd_alt(acc, inf, yneg, f30_unpack(x.l), f30_unpack(y.l), signs[b + i] != 0);
        }
        if (phi_pending && !inf) xyzz30_apply_phi(acc);
        if (!inf) {
            acc28 = xyzz30_to_xyzz28(acc);
            met = xyzz30_met_equal_x(acc28) ? 1 : 0;
        }
        if (met && form == 2) chain28(acc28, inf, yneg, pts + b, signs + b, at_inf + b, len, phi);
    }
    xyzz28_fix_sign(acc28, inf, yneg);
    out[c] = store_xyzz(acc28, inf);
    met_out[c] = met;
}

// ---- the co-Z table {P, 3P, 5P, 7P} and its phi images, mapped home (Z = Zc): out[(4 item + lane) * 16 + e],
// e = 0..3 entries and 4..7 phi images from eat28_build_quad (coz28_addu_quad inside), 8..15 the same from
// eat28_build.  Finite points of the prime-order subgroup only. ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_eat)(G1Jac *out, const G1Jac *p, int n) {
    int item, ql;
    const bool live = quad_item(n, item, ql);
    bool pi;
    const XYZZ28 xp = load_xyzz(p[item], pi);
    EAT28 tq[4], t1[4];
    F28<1, 2> zq, z1;
    quad::eat28_build_quad(tq, zq, xp, ql);
    eat28_build(t1, z1, xp);
    if (!live) return;
    G1Jac *o = out + (4 * (size_t)item + ql) * 16;
    for (int h = 0; h < 2; h++) {
        const EAT28 *t = h ? t1 : tq;
        const F28<1, 2> z = h ? z1 : zq;
        for (int m = 0; m < 4; m++) {
            JAC28 j;
            j.y = widen<1, 34>(t[m].y);
            j.z = widen<2, 4>(z);
            j.x = widen<1, 34>(t[m].x);
            o[8 * h + m] = store_jac(j, false);
            j.x = widen<1, 34>(t[m].bx);
            o[8 * h + 4 + m] = store_jac(j, false);
        }
    }
}

// ---- the digit recoding of the pipelined ladders, one thread per item: naf2_128 on k (4 words), then naf_masks on
// the digits of item i (chain 0) and of item (i + 1) % n (chain 1).  digits: NAF2_LEN per item; masks: 13 uint64 per
// item -- nz[0][0..2] neg[0][0..2] nz[1][0..2] neg[1][0..2] top (two's complement) ----
__global__ __launch_bounds__(MAX_BLOCK) void DS(k_naf)(int8_t *digits, uint64_t *masks, const uint32_t *k, int n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    const size_t i2 = (i + 1) % (size_t)n;
    int8_t d1[quad::NAF2_LEN], d2[quad::NAF2_LEN];
    quad::naf2_128(d1, k + 4 * i);
    quad::naf2_128(d2, k + 4 * i2);
    const quad::NafMasks m = quad::naf_masks(d1, d2);
    for (int j = 0; j < quad::NAF2_LEN; j++) digits[quad::NAF2_LEN * i + j] = d1[j];
    uint64_t *o = masks + 13 * i;
    for (int c = 0; c < 2; c++)
        for (int w = 0; w < 3; w++) {
            o[6 * c + w] = m.nz[c][w];
            o[6 * c + 3 + w] = m.neg[c][w];
        }
    o[12] = (uint64_t)(int64_t)m.top;
}

// ---- workgroup folds: T points per workgroup -> out[blockIdx.x].  QUAD: block_reduce_xyzz28_quad<T>, else
// dev::block_reduce_xyzz28<T> ----
template <int T, bool QUAD>
__global__ __launch_bounds__(T) void DS(k_reduce)(G1Jac *out, const G1Jac *pts) {
    __shared__ uint32_t sh[57][QUAD ? T : T / 2];
    bool inf;
    XYZZ28 acc = load_xyzz(pts[blockIdx.x * (size_t)T + threadIdx.x], inf);
    if constexpr (QUAD) quad::block_reduce_xyzz28_quad<T>(acc, inf, sh);
    else dev::block_reduce_xyzz28<T>(acc, inf, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = store_xyzz(acc, inf);
}

// ---- exported C functions ----
extern "C" {

const char *DS(f28_ops)() { return f28test::desc(); }

int DS(field)(int op, uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, int n, int block) {
    if (!geometry_ok(n, block)) return DS_BAD_ARG;
    const size_t bytes = (size_t)n * 14 * 4;
    std::vector<Arg> args = {{nullptr, out, bytes}, {a, nullptr, bytes}, {b, nullptr, bytes}, {c, nullptr, bytes}, {d, nullptr, bytes}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_field), dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, op, (uint32_t *)args[0].dev,
                           (const uint32_t *)args[1].dev, (const uint32_t *)args[2].dev, (const uint32_t *)args[3].dev,
                           (const uint32_t *)args[4].dev, n);
    });
}

int DS(f28_inv)(uint32_t *out, const uint32_t *a, int n, int block) {
    if (!geometry_ok(n, block)) return DS_BAD_ARG;
    const size_t bytes = (size_t)n * 14 * 4;
    std::vector<Arg> args = {{nullptr, out, bytes}, {a, nullptr, bytes}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_f28_inv), dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, (uint32_t *)args[0].dev,
                           (const uint32_t *)args[1].dev, n);
    });
}

static unsigned quad_grid(int n, int block) { return (unsigned)((4 * (size_t)n + block - 1) / block); }

int DS(g1_add)(int kind, G1Jac *out, uint8_t *zzok, const G1Jac *a, const G1Jac *b, const uint8_t *flags, int n, int block) {
    if (!geometry_ok(n, block) || kind < 0 || kind > 9) return DS_BAD_ARG;
    std::vector<Arg> args = {{nullptr, out, 4 * (size_t)n * sizeof(G1Jac)}, {nullptr, zzok, 4 * (size_t)n},
                             {a, nullptr, (size_t)n * sizeof(G1Jac)}, {b, nullptr, (size_t)n * sizeof(G1Jac)}, {flags, nullptr, (size_t)n}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_add), dim3(quad_grid(n, block)), dim3(block), 0, st, kind, (G1Jac *)args[0].dev, (uint8_t *)args[1].dev,
                           (const G1Jac *)args[2].dev, (const G1Jac *)args[3].dev, (const uint8_t *)args[4].dev, n);
    });
}

int DS(g1_dbl)(int kind, G1Jac *out, uint8_t *zzok, const G1Jac *a, const uint32_t *steps, int n, int block) {
    if (!geometry_ok(n, block) || kind < 0 || kind > 3) return DS_BAD_ARG;
    std::vector<Arg> args = {{nullptr, out, 4 * (size_t)n * sizeof(G1Jac)}, {nullptr, zzok, 4 * (size_t)n},
                             {a, nullptr, (size_t)n * sizeof(G1Jac)}, {steps, nullptr, (size_t)n * 4}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_dbl), dim3(quad_grid(n, block)), dim3(block), 0, st, kind, (G1Jac *)args[0].dev, (uint8_t *)args[1].dev,
                           (const G1Jac *)args[2].dev, (const uint32_t *)args[3].dev, n);
    });
}

int DS(g1_mul)(int kind, G1Jac *out, const G1Jac *p, const uint32_t *k, int halves, int n, int block) {
    if (!geometry_ok(n, block) || kind < 0 || kind > 5) return DS_BAD_ARG;
    std::vector<Arg> args = {{nullptr, out, 4 * (size_t)n * sizeof(G1Jac)}, {p, nullptr, (size_t)n * sizeof(G1Jac)}, {k, nullptr, (size_t)n * 32}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_mul), dim3(quad_grid(n, block)), dim3(block), 0, st, kind, (G1Jac *)args[0].dev, (const G1Jac *)args[1].dev,
                           (const uint32_t *)args[2].dev, halves, n);
    });
}

int DS(g1_subgroup)(int kind, G1Jac *out, uint8_t *verdict, const G1Jac *p, int n, int block) {
    if (!geometry_ok(n, block) || kind < 0 || kind > 3) return DS_BAD_ARG;
    std::vector<Arg> args = {{nullptr, out, 4 * (size_t)n * sizeof(G1Jac)}, {nullptr, verdict, 4 * (size_t)n}, {p, nullptr, (size_t)n * sizeof(G1Jac)}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_subgroup), dim3(quad_grid(n, block)), dim3(block), 0, st, kind, (G1Jac *)args[0].dev, (uint8_t *)args[1].dev,
                           (const G1Jac *)args[2].dev, n);
    });
}

// start: n + 1 offsets into pts / signs (total = start[n] entries)
int DS(g1_chain)(int kind, G1Jac *out, const G1Jac *pts, const uint8_t *signs, const uint32_t *start, int n, int block) {
    if (!geometry_ok(n, block) || kind < 0 || kind > 1) return DS_BAD_ARG;
    for (int c = 0; c < n; c++)
        if (start[c + 1] < start[c]) return DS_BAD_ARG;
    const size_t total = start[n];
    std::vector<Arg> args = {{nullptr, out, (size_t)n * sizeof(G1Jac)}, {pts, nullptr, total * sizeof(G1Jac)}, {signs, nullptr, total},
                             {start, nullptr, ((size_t)n + 1) * 4}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_chain), dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, kind, (G1Jac *)args[0].dev,
                           (const G1Jac *)args[1].dev, (const uint8_t *)args[2].dev, (const uint32_t *)args[3].dev, n);
    });
}

// ---- Fp on 13 signed 30-bit limbs and the accumulate loop's addition on it (f30_test_ops.hpp) ----
const char *DS(f30_ops)() { return f30test::desc(); }

int DS(f30field)(int op, int32_t *out, const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int n, int block) {
    if (!geometry_ok(n, block)) return DS_BAD_ARG;
    const size_t in = (size_t)n * 13 * 4;
    std::vector<Arg> args = {{nullptr, out, (size_t)n * 14 * 4}, {a, nullptr, in}, {b, nullptr, in}, {c, nullptr, in}, {d, nullptr, in}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_f30field), dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, op, (int32_t *)args[0].dev,
                           (const int32_t *)args[1].dev, (const int32_t *)args[2].dev, (const int32_t *)args[3].dev,
                           (const int32_t *)args[4].dev, n);
    });
}

static int step30(int kind, void *out, size_t out_words, uint8_t *oflags, size_t oflag_bytes, const int32_t *state, const uint8_t *flags,
                  const uint32_t *entry, int n, int block) {
    if (!geometry_ok(n, block)) return DS_BAD_ARG;
    std::vector<Arg> args = {{nullptr, out, (size_t)n * out_words * 4}, {nullptr, oflags, (size_t)n * oflag_bytes},
                             {state, nullptr, (size_t)n * f30test::STATE_WORDS * 4}};
    if (kind == 0) {
        args.push_back({flags, nullptr, (size_t)n * 3});
        args.push_back({entry, nullptr, (size_t)n * f30test::ENTRY_WORDS * 4});
    }
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_step30), dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, kind, (int32_t *)args[0].dev,
                           (uint8_t *)args[1].dev, (const int32_t *)args[2].dev, kind == 0 ? (const uint8_t *)args[3].dev : nullptr,
                           kind == 0 ? (const uint32_t *)args[4].dev : nullptr, n);
    });
}

// state: 52 int32 per item; flags: (inf, yneg, dneg) per item; entry: 24 words per item; oflags: (inf, yneg) per item
int DS(madd30_step)(int32_t *out, uint8_t *oflags, const int32_t *state, const uint8_t *flags, const uint32_t *entry, int n, int block) {
    return step30(0, out, f30test::STATE_WORDS, oflags, 2, state, flags, entry, n, block);
}
int DS(phi30)(int32_t *out, const int32_t *state, int n, int block) {
    std::vector<uint8_t> unused((size_t)(n > 0 ? n : 1));
    return step30(1, out, f30test::STATE_WORDS, unused.data(), 1, state, nullptr, nullptr, n, block);
}
// out: 56 words per item (x, y, zz, zzz of the XYZZ28); met: one byte per item
int DS(exit30)(uint32_t *out, uint8_t *met, const int32_t *state, int n, int block) {
    return step30(2, out, f30test::EXIT_WORDS, met, 1, state, nullptr, nullptr, n, block);
}

// start: n + 1 offsets into pts / signs / at_inf (total = start[n] entries); phi_at: one per chain
int DS(g1_chain30)(int form, G1Jac *out, uint8_t *met, const G1Jac *pts, const uint8_t *signs, const uint8_t *at_inf, const uint32_t *start,
                   const uint32_t *phi_at, int n, int block) {
    if (!geometry_ok(n, block) || form < 0 || form > 2) return DS_BAD_ARG;
    for (int c = 0; c < n; c++)
        if (start[c + 1] < start[c]) return DS_BAD_ARG;
    const size_t total = start[n];
    std::vector<Arg> args = {{nullptr, out, (size_t)n * sizeof(G1Jac)}, {nullptr, met, (size_t)n}, {pts, nullptr, total * sizeof(G1Jac)},
                             {signs, nullptr, total}, {at_inf, nullptr, total}, {start, nullptr, ((size_t)n + 1) * 4},
                             {phi_at, nullptr, (size_t)n * 4}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_chain30), dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, form, (G1Jac *)args[0].dev,
                           (uint8_t *)args[1].dev, (const G1Jac *)args[2].dev, (const uint8_t *)args[3].dev, (const uint8_t *)args[4].dev,
                           (const uint32_t *)args[5].dev, (const uint32_t *)args[6].dev, n);
    });
}

int DS(g1_eat)(G1Jac *out, const G1Jac *p, int n, int block) {
    if (!geometry_ok(n, block)) return DS_BAD_ARG;
    std::vector<Arg> args = {{nullptr, out, 64 * (size_t)n * sizeof(G1Jac)}, {p, nullptr, (size_t)n * sizeof(G1Jac)}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_eat), dim3(quad_grid(n, block)), dim3(block), 0, st, (G1Jac *)args[0].dev, (const G1Jac *)args[1].dev, n);
    });
}

// k: 4 words per item; digits: n * NAF2_LEN bytes; masks: n * 13 uint64 (k_naf)
int DS(naf)(int8_t *digits, uint64_t *masks, const uint32_t *k, int n, int block) {
    if (!geometry_ok(n, block)) return DS_BAD_ARG;
    std::vector<Arg> args = {{nullptr, digits, (size_t)n * quad::NAF2_LEN}, {nullptr, masks, (size_t)n * 13 * 8}, {k, nullptr, (size_t)n * 16}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(DS(k_naf), dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, (int8_t *)args[0].dev,
                           (uint64_t *)args[1].dev, (const uint32_t *)args[2].dev, n);
    });
}

// groups * threads points in, one sum per group out; (threads, quad) must be a fold the product instantiates
int DS(g1_reduce)(G1Jac *out, const G1Jac *pts, int groups, int threads, int quad_form) {
    if (groups <= 0) return DS_BAD_ARG;
    const bool q64 = quad_form && threads == 64, q256 = quad_form && threads == 256, l64 = !quad_form && threads == 64;
    if (!q64 && !q256 && !l64) return DS_BAD_ARG;
    std::vector<Arg> args = {{nullptr, out, (size_t)groups * sizeof(G1Jac)}, {pts, nullptr, (size_t)groups * threads * sizeof(G1Jac)}};
    return run_bounded(args, [&](hipStream_t st) {
        G1Jac *o = (G1Jac *)args[0].dev;
        const G1Jac *p = (const G1Jac *)args[1].dev;
        if (q64) hipLaunchKernelGGL((DS(k_reduce)<64, true>), dim3(groups), dim3(64), 0, st, o, p);
        else if (q256) hipLaunchKernelGGL((DS(k_reduce)<256, true>), dim3(groups), dim3(256), 0, st, o, p);
        else hipLaunchKernelGGL((DS(k_reduce)<64, false>), dim3(groups), dim3(64), 0, st, o, p);
    });
}

}  // extern "C"
