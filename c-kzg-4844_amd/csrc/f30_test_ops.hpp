// f30_test_ops.hpp -- the F30 field operations (fp30.hpp) at the bound combinations the accumulate loop's mixed
// addition (g1_30.hpp) instantiates, and that addition itself on raw state, behind one raw-limb calling convention
// (test aid, the 30-bit counterpart of f28_test_ops.hpp: host_shim.cpp runs it as g++ builds it,
// tests/native/dev_shim.hip as the device compiler does, with and without CKZG_F28_ASM_BLOCKS).
//
// Field.  An operand is 13 int32 limbs taken as they come, so a test can pass limbs anywhere up to LB * 2^29 in
// magnitude; `unpack` takes 12 uint32 words in their place (the 13th is not read).  A result is 14 words, unused words
// zero.  In F30<LB, VB> the value bound changes no code, it only feeds the static_asserts: the list pins the
// combinations the law relies on and tells the tests (f30test::desc()) which bounds to draw operands from.
//   mul       <1>x<1> u2, tt, zz3, zzz3, entry, exit   <5>x<1> ppp   <4>x<1> q, phi   <17>x<18> the widest pair the assert admits
//   sqr       <5> pp   <2> rr   <17> the widest
//   mul_add2  <2><5><1><1> w3   <17><17><5><5>: VA VB + VC VD = 314 exactly
//   norm      <2,5> p, d   <2,2> r   <2,4> x3 (the LA <= 2 carry formula)   <3,3> t1   <3,200> the widest (the LA = 3 one)
//             <1,1> an operand that is normalised already
//   add       <1,1>+<1,1> r, 2q   <1,1>+<2,2> t1        sub  <1,1>-<1,4> p, d   <1,1>-<1,3> x3
//   neg, unpack, to_f28; const: F30_P, F30_R392, F30_R394, F30_BETA390 (a[0] = 0..3) and F30_NINV (a[0] = 4)
//
// Addition.  Raw state: 52 int32 (x, w, zz, zzz: 4 x 13 limbs) and the flags inf, yneg.  A table entry is 24 packed
// words (x, y: 12 each), fully reduced, 2^392 domain, as the kernel gathers it.
#pragma once
#include "g1_30.hpp"

#define CKZG_F30_TEST_OPS                                                                                          \
    OP_MUL(1, 1) OP_MUL(5, 1) OP_MUL(4, 1) OP_MUL(17, 18)                                                          \
    OP_SQR(5) OP_SQR(2) OP_SQR(17)                                                                                 \
    OP_MUL_ADD2(2, 5, 1, 1) OP_MUL_ADD2(17, 17, 5, 5)                                                              \
    OP_NORM(1, 1) OP_NORM(2, 5) OP_NORM(2, 2) OP_NORM(2, 4) OP_NORM(3, 3) OP_NORM(3, 200)                          \
    OP_ADD(1, 1, 1, 1) OP_ADD(1, 1, 2, 2) OP_SUB(1, 1, 1, 4) OP_SUB(1, 1, 1, 3)                                    \
    OP_NEG(1) OP_UNPACK() OP_TO_F28() OP_CONST()

namespace ckzg {
namespace f30test {

constexpr int STATE_WORDS = 52;   // x, w, zz, zzz
constexpr int ENTRY_WORDS = 24;   // x, y packed
constexpr int EXIT_WORDS = 56;    // x, y, zz, zzz of an XYZZ28

template <int L, int V>
HD F30<L, V> ld(const int32_t *p) {
    F30<L, V> r;
#pragma unroll
    for (int j = 0; j < 13; j++) r.l[j] = p[j];
    return r;
}
template <int L, int V>
HD void st(int32_t *o, const F30<L, V> &v) {
#pragma unroll
    for (int j = 0; j < 13; j++) o[j] = v.l[j];
    o[13] = 0;
}
template <int L, int V>
HD void st(int32_t *o, const F28<L, V> &v) {
#pragma unroll
    for (int j = 0; j < 14; j++) o[j] = (int32_t)v.l[j];
}

HD void st_const(int32_t *o, int which) {
#pragma unroll
    for (int j = 0; j < 14; j++) o[j] = 0;
#pragma unroll
    for (int j = 0; j < 13; j++) {
        if (which == 0) o[j] = F30_P[j];
        else if (which == 1) o[j] = F30_R392[j];
        else if (which == 2) o[j] = F30_R394[j];
        else if (which == 3) o[j] = F30_BETA390[j];
    }
    if (which == 4) o[0] = (int32_t)F30_NINV;
}

// operation number `op` of the list on one item: o <- op(a, b, c, d); returns false for a number past the list
HDNI inline bool run(int op, int32_t *o, const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d) {
    int n = 0;
#define OP_MUL(VA, VB) if (op == n++) { st(o, mul(ld<1, VA>(a), ld<1, VB>(b))); return true; }
#define OP_SQR(VA) if (op == n++) { st(o, sqr(ld<1, VA>(a))); return true; }
#define OP_MUL_ADD2(VA, VB, VC, VD) \
    if (op == n++) { st(o, mul_add2(ld<1, VA>(a), ld<1, VB>(b), ld<1, VC>(c), ld<1, VD>(d))); return true; }
#define OP_NORM(LA, VA) if (op == n++) { st(o, norm(ld<LA, VA>(a))); return true; }
#define OP_ADD(LA, VA, LB, VB) if (op == n++) { st(o, add(ld<LA, VA>(a), ld<LB, VB>(b))); return true; }
#define OP_SUB(LA, VA, LB, VB) if (op == n++) { st(o, sub(ld<LA, VA>(a), ld<LB, VB>(b))); return true; }
#define OP_NEG(V) if (op == n++) { st(o, f30_neg(ld<1, V>(a))); return true; }
#define OP_UNPACK() if (op == n++) { uint32_t w[12]; for (int j = 0; j < 12; j++) w[j] = (uint32_t)a[j]; st(o, f30_unpack(w)); return true; }
#define OP_TO_F28() if (op == n++) { st(o, f30_to_f28(ld<1, 1>(a))); return true; }
#define OP_CONST() if (op == n++) { st_const(o, a[0]); return true; }
    CKZG_F30_TEST_OPS
#undef OP_MUL
#undef OP_SQR
#undef OP_MUL_ADD2
#undef OP_NORM
#undef OP_ADD
#undef OP_SUB
#undef OP_NEG
#undef OP_UNPACK
#undef OP_TO_F28
#undef OP_CONST
    return false;
}

// one line per operation, in order: its name and template arguments
inline const char *desc() {
    return ""
#define OP_MUL(VA, VB) "mul " #VA " " #VB "\n"
#define OP_SQR(VA) "sqr " #VA "\n"
#define OP_MUL_ADD2(VA, VB, VC, VD) "mul_add2 " #VA " " #VB " " #VC " " #VD "\n"
#define OP_NORM(LA, VA) "norm " #LA " " #VA "\n"
#define OP_ADD(LA, VA, LB, VB) "add " #LA " " #VA " " #LB " " #VB "\n"
#define OP_SUB(LA, VA, LB, VB) "sub " #LA " " #VA " " #LB " " #VB "\n"
#define OP_NEG(V) "neg " #V "\n"
#define OP_UNPACK() "unpack\n"
#define OP_TO_F28() "to_f28\n"
#define OP_CONST() "const\n"
        CKZG_F30_TEST_OPS
#undef OP_MUL
#undef OP_SQR
#undef OP_MUL_ADD2
#undef OP_NORM
#undef OP_ADD
#undef OP_SUB
#undef OP_NEG
#undef OP_UNPACK
#undef OP_TO_F28
#undef OP_CONST
        ;
}

// ---- the addition on raw state ----
HD void ld_state(XYZZ30 &acc, const int32_t *s) {
    acc.x = ld<1, 4>(s);
    acc.w = ld<1, 1>(s + 13);
    acc.zz = ld<1, 1>(s + 26);
    acc.zzz = ld<1, 1>(s + 39);
}
HD void st_state(int32_t *o, const XYZZ30 &acc) {
#pragma unroll
    for (int j = 0; j < 13; j++) {
        o[j] = acc.x.l[j];
        o[13 + j] = acc.w.l[j];
        o[26 + j] = acc.zz.l[j];
        o[39 + j] = acc.zzz.l[j];
    }
}

// xyzz30_madd_alt.  flags in: inf, yneg, dneg; flags out: inf, yneg.  An empty accumulator's limbs are not read by
// the law, but they travel: the state is loaded whatever `inf` says.
HDNI inline void madd_step(int32_t *o, uint8_t *oflags, const int32_t *s, const uint8_t *flags, const uint32_t *entry) {
    XYZZ30 acc;
    ld_state(acc, s);
    bool inf = flags[0] != 0, yneg = flags[1] != 0;
    xyzz30_madd_alt(acc, inf, yneg, f30_unpack(entry), f30_unpack(entry + 12), flags[2] != 0);
    st_state(o, acc);
    oflags[0] = inf ? 1 : 0;
    oflags[1] = yneg ? 1 : 0;
}

HDNI inline void phi_step(int32_t *o, const int32_t *s) {
    XYZZ30 acc;
    ld_state(acc, s);
    xyzz30_apply_phi(acc);
    st_state(o, acc);
}

// xyzz30_to_xyzz28 (x, y, zz, zzz: 4 x 14 words) and xyzz30_met_equal_x
HDNI inline void exit_step(uint32_t *o, uint8_t *met, const int32_t *s) {
    XYZZ30 acc;
    ld_state(acc, s);
    const XYZZ28 r = xyzz30_to_xyzz28(acc);
#pragma unroll
    for (int j = 0; j < 14; j++) {
        o[j] = r.x.l[j];
        o[14 + j] = r.y.l[j];
        o[28 + j] = r.zz.l[j];
        o[42 + j] = r.zzz.l[j];
    }
    *met = xyzz30_met_equal_x(r) ? 1 : 0;
}

}  // namespace f30test
}  // namespace ckzg
