// fr_lds.hpp -- an Fr vector in LDS and an Fr as canonical limbs, for the kernels of coset_verify.hip and
// coset_groups.hip.
#pragma once
#include "device.hpp"

namespace ckzg {
namespace dev {

// An Fr vector in LDS, limb-major: limb k of element i at sh[k * n + i], so that the lanes of a wave that read
// consecutive elements read consecutive words (element-major, 32 B apart, eight lanes would share a bank).
template <uint32_t N>
__device__ __forceinline__ Fr lds_ld(const uint32_t *sh, uint32_t i) {
    Fr r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = sh[k * N + i];
    return r;
}
template <uint32_t N>
__device__ __forceinline__ void lds_st(uint32_t *sh, uint32_t i, const Fr &v) {
#pragma unroll
    for (int k = 0; k < 8; k++) sh[k * N + i] = v.l[k];
}

__device__ __forceinline__ void store_raw(uint32_t *out, const Fr &v) {
    uint32_t a[8];
    to_raw<FrParams>(a, v);
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = a[k];
}

}  // namespace dev
}  // namespace ckzg
