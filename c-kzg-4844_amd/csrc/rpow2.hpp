// rpow2.hpp -- the powers of a batch challenge, made where they are used: only r crosses PCIe (verify.hip:
// k_rlc_scalars; coset_verify.hip: k_coset_rlc_scalars; coset_groups.hip: k_coset_group_rlc_scalars; locate.hip:
// k_locate_scale).
#pragma once
#include "field.hpp"

namespace ckzg {
namespace dev {

// r^(2^k), k < 24, made on the host (23 squarings) and passed by value: a lane's power of r is then the product of
// the entries its index selects -- <= 13 products for n = 8192, ~6 on average, and no squarings of its own.
struct RPow2 {
    Fr p[24];
};
__device__ __forceinline__ Fr rpow_at(const RPow2 &t, uint32_t i) {
    Fr pw = Fr::one();
    bool first = true;
#pragma unroll 1
    for (int k = 0; k < 24 && (i >> k); k++) {
        if ((i >> k) & 1u) {
            pw = first ? t.p[k] : mul(pw, t.p[k]);
            first = false;
        }
    }
    return pw;
}
inline RPow2 rpow2_of(const Fr &r) {
    RPow2 t;
    t.p[0] = r;
    for (int k = 1; k < 24; k++) t.p[k] = mul(t.p[k - 1], t.p[k - 1]);
    return t;
}

}  // namespace dev
}  // namespace ckzg
