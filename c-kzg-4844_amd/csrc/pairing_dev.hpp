// pairing_dev.hpp -- the BLS12-381 pairing check against two FIXED G2 arguments, for one lane of a GPU kernel
// (pairing.hip: k_pairing_check) and, compiled by g++, for the host shims that test it (field_test_ops.hpp).
//
// The tower, the sparse line product and the final exponentiation are tower.hpp's, shared with the host's pairing
// (host_pairing.hpp).  What is the device's own is the Miller product: it reads the lam[] and c[] arrays of
// host_pairing.hpp's G2Prepared line tables as they were uploaded, and keeps the lanes of a wave together by selecting
// where the host branches.
#pragma once
#include "tower.hpp"

namespace ckzg {
namespace pdev {
using namespace tower;

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

// The Miller-loop value of e(p1, Q1) * e(p2, Q2) with Q1, Q2 given by their line tables (MILLER_STEPS entries each).
// An infinite G1 argument makes its factor 1 (host_pairing.hpp: miller_product_prepared): here every line product is
// computed and the lane's infinity flag SELECTS whether it is kept, so that the lanes of a wave never diverge.  Every lane
// reads the same table step at the same time: the loads are wave-uniform.
HDNI inline Fp12 miller_product_tables(const G1Affine &p1, const LineTable &q1, const G1Affine &p2, const LineTable &q2) {
    const uint32_t use1 = p1.is_inf() ? 0u : ~0u, use2 = p2.is_inf() ? 0u : ~0u;
    Fp12 f = Fp12::one();
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

// e(p1, Q1) * e(p2, Q2) == 1 ?
HDNI inline bool pairing_product_is_one(const G1Affine &p1, const LineTable &q1, const G1Affine &p2, const LineTable &q2) {
    return is_one(final_exp(miller_product_tables(p1, q1, p2, q2)));
}

}  // namespace pdev
}  // namespace ckzg
