// fr_inv.hpp -- inversion in Fr by the safegcd divstep iteration of fp28_inv.hpp (safegcd30<Safegcd30Fr>), on 9 signed
// 30-bit limbs (255-bit modulus).  The barycentric evaluation inverts one product per lane; the
// Fermat ladder there (255 squarings + ~127 products) was four fifths of the kernel.  Bound: 738
// divsteps suffice for 255-bit inputs, i.e. at most 25 batches of 30; |d|, |e| grow by at most r per
// batch and 9 x 30 bits hold 2^14 r.  Here: the 32-bit words in and out, and the product that restores the radix.
#pragma once
#include "fp28_inv.hpp"

namespace ckzg {

// 1/a for a in Montgomery form (radix 2^256), result in Montgomery form; 0 for a == 0
HDNI inline Fr fr_inv_safegcd(const Fr &a) {
    if (a.is_zero()) return Fr::zero();
    int32_t g[9];
    for (int i = 0; i < 9; i++) {
        int bit = 30 * i, j = bit >> 5, sh = bit & 31;
        uint32_t v = j < 8 ? a.l[j] >> sh : 0u;
        if (sh > 2 && j + 1 < 8) v |= a.l[j + 1] << (32 - sh);
        g[i] = (int32_t)(v & 0x3fffffffu);
    }
    uint32_t w[9];
    safegcd30<Safegcd30Fr>(w, g);
    // 9 x 30 -> 32-bit words: y = lo + hi * 2^256 with hi < 2^5 (y < 59r < 2^261)
    uint32_t raw[9];
    for (int k = 0; k < 9; k++) {
        int bit = 32 * k, i = bit / 30, sh = bit - 30 * i;
        uint64_t v = (uint64_t)w[i] >> sh;
        if (i + 1 < 9) v |= (uint64_t)w[i + 1] << (30 - sh);
        raw[k] = (uint32_t)v;
    }
    // y = 1/(a R) as an integer; the Montgomery form of 1/a is y R^2 = mul(lo, R^3) + mul(hi R, R^3)
    Fr lo, r3;
    for (int k = 0; k < 8; k++) {
        lo.l[k] = raw[k];
        r3.l[k] = FR_R3[k];
    }
    Fr res = mul(lo, r3);
    if (raw[8]) res = add(res, mul(fr_from_u64(raw[8]), r3));
    return res;
}

}  // namespace ckzg
