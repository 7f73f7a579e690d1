// f28_test_ops.hpp -- the F28 field operations at the bound combinations the group law instantiates, behind one
// raw-limb calling convention (test aid: host_shim.cpp runs it as g++ builds it, tests/native/dev_shim.hip as the
// device compiler does, with and without CKZG_F28_ASM_BLOCKS).  An operand is 14 uint32 limbs taken as they come,
// so a test can pass limbs anywhere below LB * 2^28; a result is 14 words (a field element), 12 words (an Fp) or one
// word (a predicate).  The list is the single source of the instantiations: f28test::desc() spells it out for the
// tests, which draw their inputs from the bounds named there.
//
// Where each combination comes from (g1_28.hpp, g1_quad.hpp, g1_pipe.hpp; "239" / "255" are the column-accumulator
// budgets 14*LA*LB+15 and 15*LA*LA+15 the headers annotate):
//   mul   <4,64>x<4,6>  jac28_add_quad step 3 (239)      <4,6>x<4,18>   its step 5, xyzz28_add_quad step 4 (239)
//         <4,6>x<4,6>   step 4 / xyzz28_add_quad step 2  <3,34>x<3,34>  jac28_dbl_quad step 2 (14*9+15)
//         <2,34>x<2,34> jac28_dbl_quad step 1            <2,34>x<2,4>   jac28_add_quad step 1
//         <4,41>x<4,37>, <4,37>x<4,37>, <4,37>x<4,18>, <2,41>x<2,41>    jac28_madd_quad_zz steps B, C, D, A
//         <4,41>x<4,41>, <4,41>x<4,18>  coz28_addu_quad steps 1, 3      <4,10>x<4,18>  xyzz28_madd r*d (239)
//         <3,6>x<4,18>  xyzz28_dbl_affine m*d            <3,6>x<1,72>   jac28_dbl E*dx
//   sqr   <4,6> jac28_add h (255)   <4,41> coz28_addu dX (255, the widest value at four units)   <4,23> je28_madd
//         <4,18> xyzz28_madd p   <3,6> jac28_dbl E (15*9+15)   <2,12> xyzz28_dbl   <2,8> xyzz28_madd_alt r
//   mul_add2  <2,8><4,18><1,6><1,2> xyzz28_madd_alt    <1,6><4,18><4,4><1,2> jac28_add, xyzz28_add
//             <3,6><4,18><1,2><4,8> xyzz28_dbl (239)   <1,23><4,18><3,21><1,2> je28_madd
//   sub   <1,0>-<1,34> jac28_add_quad_pipe's -Y (K = 64, the largest multiple of p any routine adds)
//   sub_k <35> <1,2>-<1,34> and <1,0>-<1,34>: jac28_madd_quad_zz's h, r (results <4,37>) and -Y1 (<3,35>)
#pragma once
#include "g1_28.hpp"

#define CKZG_F28_TEST_OPS                                                                                          \
    OP_MUL(4, 64, 4, 6) OP_MUL(4, 6, 4, 18) OP_MUL(4, 6, 4, 6) OP_MUL(3, 34, 3, 34) OP_MUL(2, 34, 2, 34)           \
    OP_MUL(2, 34, 2, 4) OP_MUL(4, 41, 4, 37) OP_MUL(4, 37, 4, 37) OP_MUL(4, 37, 4, 18) OP_MUL(2, 41, 2, 41)        \
    OP_MUL(4, 41, 4, 41) OP_MUL(4, 41, 4, 18) OP_MUL(4, 10, 4, 18) OP_MUL(3, 6, 4, 18) OP_MUL(3, 6, 1, 72)         \
    OP_MUL(4, 18, 1, 2) OP_MUL(4, 2, 1, 2) OP_MUL(1, 1, 1, 2) OP_MUL(1, 2, 1, 2)                                   \
    OP_SQR(4, 6) OP_SQR(4, 41) OP_SQR(4, 23) OP_SQR(4, 18) OP_SQR(3, 6) OP_SQR(2, 12) OP_SQR(2, 8) OP_SQR(2, 4)    \
    OP_SQR(1, 34) OP_SQR(1, 20) OP_SQR(1, 2)                                                                       \
    OP_MUL_ADD2(2, 8, 4, 18, 1, 6, 1, 2) OP_MUL_ADD2(1, 6, 4, 18, 4, 4, 1, 2) OP_MUL_ADD2(3, 6, 4, 18, 1, 2, 4, 8) \
    OP_MUL_ADD2(1, 23, 4, 18, 3, 21, 1, 2) OP_MUL_ADD2(1, 2, 1, 2, 1, 2, 1, 2)                                     \
    OP_ADD(1, 2, 1, 2) OP_ADD(2, 4, 2, 4) OP_ADD(4, 8, 4, 8) OP_ADD(1, 2, 1, 6) OP_ADD(1, 2, 2, 4)                 \
    OP_SUB(1, 2, 1, 2) OP_SUB(1, 2, 1, 10) OP_SUB(1, 2, 1, 6) OP_SUB(1, 2, 3, 6) OP_SUB(1, 2, 8, 16)               \
    OP_SUB(4, 8, 1, 34) OP_SUB(1, 0, 1, 6) OP_SUB(1, 0, 1, 1) OP_SUB(1, 0, 1, 34)                                  \
    OP_SUB_K(21, 1, 20, 1, 20) OP_SUB_K(35, 1, 2, 1, 34) OP_SUB_K(17, 1, 2, 8, 16) OP_SUB_K(20, 4, 8, 1, 19)       \
    OP_SUB_K(21, 1, 0, 1, 20) OP_SUB_K(35, 1, 0, 1, 34)                                                            \
    OP_NORM(11, 34) OP_NORM(7, 72) OP_NORM(6, 10) OP_NORM(4, 6) OP_NORM(8, 4) OP_NORM(2, 4) OP_NORM(4, 64)         \
    OP_TO_FP(1, 2) OP_TO_FP(1, 10) OP_TO_FP(4, 64)                                                                 \
    OP_FROM_FP() OP_CNEG() OP_IS_ZERO() OP_EQUAL(1, 2, 1, 2) OP_EQUAL(1, 34, 1, 2)

namespace ckzg {
namespace f28test {

template <int L, int V>
HD F28<L, V> ld(const uint32_t *p) {
    F28<L, V> r;
#pragma unroll
    for (int j = 0; j < 14; j++) r.l[j] = p[j];
    return r;
}
template <int L, int V>
HD void st(uint32_t *o, const F28<L, V> &v) {
#pragma unroll
    for (int j = 0; j < 14; j++) o[j] = v.l[j];
}
HD void st(uint32_t *o, const Fp &v) {
#pragma unroll
    for (int j = 0; j < 12; j++) o[j] = v.l[j];
    o[12] = o[13] = 0;
}
HD void st(uint32_t *o, bool v) {
    o[0] = v ? 1u : 0u;
#pragma unroll
    for (int j = 1; j < 14; j++) o[j] = 0;
}

// operation number `op` of the list on one item: o <- op(a, b, c, d); returns false for a number past the list
HDNI inline bool run(int op, uint32_t *o, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d) {
    int n = 0;
#define OP_MUL(LA, VA, LB, VB) if (op == n++) { st(o, mul(ld<LA, VA>(a), ld<LB, VB>(b))); return true; }
#define OP_SQR(LA, VA) if (op == n++) { st(o, sqr(ld<LA, VA>(a))); return true; }
#define OP_MUL_ADD2(LA, VA, LB, VB, LC, VC, LD, VD) \
    if (op == n++) { st(o, mul_add2(ld<LA, VA>(a), ld<LB, VB>(b), ld<LC, VC>(c), ld<LD, VD>(d))); return true; }
#define OP_ADD(LA, VA, LB, VB) if (op == n++) { st(o, add(ld<LA, VA>(a), ld<LB, VB>(b))); return true; }
#define OP_SUB(LA, VA, LB, VB) if (op == n++) { st(o, sub(ld<LA, VA>(a), ld<LB, VB>(b))); return true; }
#define OP_SUB_K(K, LA, VA, LB, VB) if (op == n++) { st(o, sub_k<K>(ld<LA, VA>(a), ld<LB, VB>(b))); return true; }
#define OP_NORM(LA, VA) if (op == n++) { st(o, norm(ld<LA, VA>(a))); return true; }
#define OP_TO_FP(LA, VA) if (op == n++) { st(o, f28_to_fp(ld<LA, VA>(a))); return true; }
#define OP_FROM_FP() if (op == n++) { Fp x; for (int j = 0; j < 12; j++) x.l[j] = a[j]; st(o, f28_from_fp(x)); return true; }
#define OP_CNEG() if (op == n++) { st(o, cneg_reduced(ld<1, 1>(a), b[0] != 0)); return true; }
#define OP_IS_ZERO() if (op == n++) { st(o, is_zero(ld<1, 2>(a))); return true; }
#define OP_EQUAL(LA, VA, LB, VB) if (op == n++) { st(o, f28_equal(ld<LA, VA>(a), ld<LB, VB>(b))); return true; }
    CKZG_F28_TEST_OPS
#undef OP_MUL
#undef OP_SQR
#undef OP_MUL_ADD2
#undef OP_ADD
#undef OP_SUB
#undef OP_SUB_K
#undef OP_NORM
#undef OP_TO_FP
#undef OP_FROM_FP
#undef OP_CNEG
#undef OP_IS_ZERO
#undef OP_EQUAL
    return false;
}

// one line per operation, in order: its name and template arguments
inline const char *desc() {
    return ""
#define OP_MUL(LA, VA, LB, VB) "mul " #LA " " #VA " " #LB " " #VB "\n"
#define OP_SQR(LA, VA) "sqr " #LA " " #VA "\n"
#define OP_MUL_ADD2(LA, VA, LB, VB, LC, VC, LD, VD) "mul_add2 " #LA " " #VA " " #LB " " #VB " " #LC " " #VC " " #LD " " #VD "\n"
#define OP_ADD(LA, VA, LB, VB) "add " #LA " " #VA " " #LB " " #VB "\n"
#define OP_SUB(LA, VA, LB, VB) "sub " #LA " " #VA " " #LB " " #VB "\n"
#define OP_SUB_K(K, LA, VA, LB, VB) "sub_k " #K " " #LA " " #VA " " #LB " " #VB "\n"
#define OP_NORM(LA, VA) "norm " #LA " " #VA "\n"
#define OP_TO_FP(LA, VA) "to_fp " #LA " " #VA "\n"
#define OP_FROM_FP() "from_fp\n"
#define OP_CNEG() "cneg\n"
#define OP_IS_ZERO() "is_zero\n"
#define OP_EQUAL(LA, VA, LB, VB) "equal " #LA " " #VA " " #LB " " #VB "\n"
        CKZG_F28_TEST_OPS
#undef OP_MUL
#undef OP_SQR
#undef OP_MUL_ADD2
#undef OP_ADD
#undef OP_SUB
#undef OP_SUB_K
#undef OP_NORM
#undef OP_TO_FP
#undef OP_FROM_FP
#undef OP_CNEG
#undef OP_IS_ZERO
#undef OP_EQUAL
        ;
}

}  // namespace f28test
}  // namespace ckzg
