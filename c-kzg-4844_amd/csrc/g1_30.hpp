// g1_30.hpp -- the accumulate loop's mixed addition on the 13 x 30-bit signed field (fp30.hpp).  The same law as
// g1_28.hpp::xyzz28_madd_alt: sign-alternating W, one fused reduction.  It lives only between the table gather and
// the workgroup fold of the throughput accumulate kernel: entry from a table coordinate, exit into an XYZZ28.
//
// The domain invariant.  Table coordinates are stored in the 2^392 Montgomery domain, x~ = x 2^392; this field
// reduces with 2^390, so a product comes out k = 4 times its 2^392-domain value.  Write [v]_e = v 2^392 k^e ("v at
// weight e"): mul30([a]_e, [b]_f) = a b 2^784 k^(e+f) / 2^390 = [a b]_(e+f+1), and sums need equal weights.
// The accumulator is held at weights (X, W, ZZ, ZZZ) = (1, 2, 0, 1); a table entry (x2, t) has weight 0.  Then
//     U2 = x2 ZZ  [1]   P = U2 - X  [1]      T = t ZZZ  [2]   R = T + W  [2]
//     PP = P^2  [3]     PPP = P PP  [5]      Q = X PP  [5]    RR = R^2  [5]
//     X3 = RR - PPP - 2Q  [5]     D = Q - X3  [5]     W3 = R D + W PPP  [8]     ZZ3 = ZZ PP  [4]     ZZZ3 = ZZZ PPP  [7]
// every sum is homogeneous, and the new weights are (5, 8, 4, 7) = (1, 2, 0, 1) + (4, 6, 4, 6): the old pattern times
// the projective rescaling (l^2, l^3, l^2, l^3) with l = k^2, under which (X, Y, ZZ, ZZZ) names the same point.  So one
// addition maps the pattern to itself and the represented point is the one the 28-bit law computes.
//   entry  (first entry copied into an empty accumulator): (mul30(x2, 2^392), mul30(t, 2^394), 2^392, 2^394)
//          = ([x2]_1, [t]_2, [1]_0, [1]_1).
//   phi    X <- mul30(X, beta 2^390) = beta X at the same weight.
//   exit   multiply by (2^392, 2^392, 2^394, 2^394): weights (2, 3, 2, 3) = (0, 0, 0, 0) + (l^2, l^3, l^2, l^3), l = k: a
//          point of the 2^392 domain.  Each of the four is a product with a constant below p, at most
//          (16/629 + 0.51) p in magnitude; f30_to_f28 adds p and repacks into [0, 2p].
//
// Equal x.  The law has no branch for P = 0 (the entry is the accumulator's point or its negative).  If some step has
// P = 0 mod p then ZZ3 = ZZ PP = 0 mod p, and ZZ stays 0 through every later step; a chain without such a step never
// has ZZ = 0, because p is prime and every factor P is a unit.  So ZZ = 0 at exit says exactly "some step had equal
// x", and the caller reruns that chain through xyzz28_madd_alt, which has the doubling and the infinity branch.
#pragma once
#include "fp30.hpp"
#include "g1_28.hpp"

namespace ckzg {

struct XYZZ30 {
    F30<1, 4> x;     // weight 1
    F30<1, 1> w;     // weight 2; +-Y, `yneg` says which
    F30<1, 1> zz;    // weight 0
    F30<1, 1> zzz;   // weight 1
};

template <int V2, int V>
HD F30<1, V2> widen30(const F30<1, V> &a) {
    static_assert(V2 >= V, "bounds can only be loosened");
    F30<1, V2> r;
#pragma unroll
    for (int j = 0; j < 13; j++) r.l[j] = a.l[j];
    return r;
}

// acc += +-(x2, y2): (x2, y2) is the table entry, fully reduced, in balanced limbs (f30_unpack); `dneg` asks for
// its negative.  Not infinity.  Equal x is NOT handled here (see above).
HD void xyzz30_madd_alt(XYZZ30 &acc, bool &inf, bool &yneg, const F30<1, 1> &x2, const F30<1, 1> &y2, bool dneg) {
    if (inf) yneg = false;
    // yneg == false: stored +Y, want t = -(+-y2); yneg == true: stored -Y, want t = +(+-y2)
    const bool tneg = dneg != !yneg;
    const F30<1, 1> ny = f30_neg(y2);
    F30<1, 1> t;
#pragma unroll
    for (int j = 0; j < 13; j++) t.l[j] = tneg ? ny.l[j] : y2.l[j];
    if (inf) {
        acc.x = widen30<4>(mul(x2, f30_const<1>(F30_R392)));
        acc.w = mul(t, f30_const<1>(F30_R394));        // = -(the point's y): stored sign is "negative"
        acc.zz = f30_const<1>(F30_R392);
        acc.zzz = f30_const<1>(F30_R394);
        inf = false;
        yneg = true;
        return;
    }
    auto u2 = mul(x2, acc.zz);                          // <1,1>
    auto tt = mul(t, acc.zzz);                          // <1,1>   -+S2
    auto p = norm(sub(u2, acc.x));                      // <2,5> -> <1,5>
    auto r = norm(add(tt, acc.w));                      // <2,2> -> <1,2>   -+R
    auto pp = sqr(p);                                   // 25 <= 314
    auto ppp = mul(p, pp);                              // 5
    auto q = mul(acc.x, pp);                            // 4
    auto rr = sqr(r);                                   // 4
    auto t1 = norm(add(ppp, add(q, q)));                // <3,3> -> <1,3>
    acc.x = norm(sub(rr, t1));                          // <2,4> -> <1,4>
    auto d = norm(sub(q, acc.x));                       // <2,5> -> <1,5>
    acc.w = mul_add2(r, d, acc.w, ppp);                 // 2*5 + 1*1 = 11
    acc.zz = mul(acc.zz, pp);
    acc.zzz = mul(acc.zzz, ppp);
    yneg = !yneg;
}

// phi on the accumulator: X scaled by beta, weight unchanged
HD void xyzz30_apply_phi(XYZZ30 &acc) { acc.x = widen30<4>(mul(acc.x, f30_const<1>(F30_BETA390))); }

// exit: the accumulator as a point of the 2^392 domain in the 28-bit form (W still +-Y: xyzz28_fix_sign comes next)
HD XYZZ28 xyzz30_to_xyzz28(const XYZZ30 &acc) {
    XYZZ28 o;
    o.x = widen<1, 10>(f30_to_f28(mul(acc.x, f30_const<1>(F30_R392))));
    o.y = widen<1, 6>(f30_to_f28(mul(acc.w, f30_const<1>(F30_R392))));
    o.zz = f30_to_f28(mul(acc.zz, f30_const<1>(F30_R394)));
    o.zzz = f30_to_f28(mul(acc.zzz, f30_const<1>(F30_R394)));
    return o;
}

// ZZ = 0 mod p at exit: some step of the chain met an entry with the accumulator's x.  `o` is xyzz30_to_xyzz28's result
// (zz normalised, in [0, 2p]; an exit product is at most 0.54 p in magnitude, so after + p it is 0 mod p only as p itself
// -- is_zero() tests 0 and p).
HD bool xyzz30_met_equal_x(const XYZZ28 &o) { return is_zero(o.zz); }

}  // namespace ckzg
