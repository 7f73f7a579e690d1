// recover_set_factors.hpp -- the vanishing polynomial of a set of missing cells, cell by cell.
//
// recover_cells (recovery.c:200-365) multiplies the extended blob by Z over the domain and divides by Z over the
// coset 7 w^i, Z being the polynomial that vanishes on the missing cells: Z(x) = short(x^64), short the product of
// (y - w128^brp7(j)) over the missing cells j, w128 = w^64 (recovery.c:46-134).  The data is held in cell
// (bit-reversed) order: position p = 64 c + k is the natural index brp13(p), whose low 7 bits are brp7(c), and x^64
// only sees those.  So Z is constant over each cell:
//   Z at every position of cell c          = prod over missing j of (w128^brp7(c)        - w128^brp7(j))
//   Z on the coset at every position of c  = prod over missing j of (7^64 w128^brp7(c)   - w128^brp7(j))
// The first is zero exactly for the missing cells, the second never (7^64 w128^a is no 128th root of unity).
// One function for the device kernel (verify.hip: k_recover_set_factors) and the host replay (host_shim.cpp).
#pragma once
#include "field.hpp"

namespace ckzg {

HD uint32_t recover_brp7(uint32_t c) {
    uint32_t o = 0;
#pragma unroll
    for (int b = 0; b < 7; b++) o |= ((c >> b) & 1u) << (6 - b);
    return o;
}

// mask: bit j of word j / 32 set = cell j is held; roots: w^i, i <= 8192; seven64 = 7^64.  Two independent chains
// of one product per missing cell (at most 64: a valid row holds at least 64 cells).
HD void recover_set_products(Fr &z_domain, Fr &z_coset, const uint32_t *mask, uint32_t c, const Fr *roots,
                             const Fr &seven64) {
    const Fr xd = roots[64u * recover_brp7(c)], xc = mul(seven64, xd);
    Fr pd = Fr::one(), pc = Fr::one();
    for (uint32_t j = 0; j < 128; j++) {
        if ((mask[j >> 5] >> (j & 31u)) & 1u) continue;
        const Fr rj = roots[64u * recover_brp7(j)];
        pd = mul(pd, sub(xd, rj));
        pc = mul(pc, sub(xc, rj));
    }
    z_domain = pd;
    z_coset = pc;
}

}  // namespace ckzg
