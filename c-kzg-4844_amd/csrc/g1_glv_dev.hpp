// g1_glv_dev.hpp -- the per-term GLV half-ladder and the complete XYZZ addition as out-of-line device functions, for the
// kernels that compute a handful of scalar multiples per lane (pairing.hip: k_point_lhs; locate.hip: k_locate_scale,
// the G1 prefix scan).  Each translation unit that includes this gets one copy of each body.
#pragma once
#include "g1_28.hpp"

namespace ckzg {
namespace dev {

// [k]P for one 128-bit GLV half (P itself, or phi(P) = (beta x, y) for the second half): the per-term ladder of
// verify.hip's k_lincomb_partial (xyzz28_mul_w4_128), one call site per half so that the ladder's code exists once
__device__ __noinline__ inline G1XYZZ glv_half_mul(const G1Affine &a, const uint32_t *k128, bool second) {
    XYZZ28 p, o;
    bool oi = true;
    p.x = widen<1, 10>(f28_from_fp(a.x));
    if (second) p.x = widen<1, 10>(mul(p.x, f28_const<1, 1>(FP28_BETA_LAMBDA)));
    p.y = widen<1, 6>(f28_from_fp(a.y));
    p.zz = widen<1, 2>(f28_one());
    p.zzz = p.zz;
    xyzz28_mul_w4_128(o, oi, p, a.is_inf(), k128);
    return xyzz28_to_xyzz(o, oi);
}

// g1.hpp's complete XYZZ addition, out of line: k_point_lhs adds four ladder results, and inlined four times the
// addition was most of the kernel's code
__device__ __noinline__ inline G1XYZZ xyzz_add_ni(const G1XYZZ &a, const G1XYZZ &b) { return xyzz_add(a, b); }

}  // namespace dev
}  // namespace ckzg
