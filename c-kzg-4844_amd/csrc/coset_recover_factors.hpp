// coset_recover_factors.hpp -- the vanishing polynomial of a set of missing cosets of size l = 2^e, coset by coset.
//
// Recovery (recovery.c:200-365) multiplies the extended blob by Z over the domain and divides by Z over the coset
// 7 w^i, Z being the polynomial that vanishes on the missing cosets: Z(x) = short(x^l), short the product of
// (y - w_m^b(j)) over the missing cosets j, w_m = w^l (recovery.c:46-134 at l = 64).  The data is held in bit-reversed
// order: position p = l c + k is the natural index brp13(p), whose low 13 - e bits are b(c) = brp_{13-e}(c), and x^l
// only sees those.  So Z is constant over each coset:
//   Z at every position of coset c          = prod over missing j of (      w_m^b(c) - w_m^b(j))
//   Z on the shifted coset, every pos. of c = prod over missing j of (7^l w_m^b(c) - w_m^b(j))
// The first is zero exactly for the missing cosets, the second never.  A set has up to m / 2 = 4096 missing cosets at
// e = 0, so the product of one coset may be split over `parts` lanes (coset_recover_plan.hpp: coset_recover_parts);
// each takes a contiguous slice of the missing list, every slice padded to the same number of steps with the factor 1.
// One function for the device kernel (coset_recover.hip: k_coset_recover_factors) and the host replay (host_shim.cpp).
#pragma once
#include "field.hpp"

namespace ckzg {

// One (coset, part), `steps` steps of its slice: pd *= prod (xd - root(t)), pc *= prod (xc - root(t)) over t < valid,
// two independent chains; steps t >= valid multiply by 1 (root(t) must still be readable).  root(t): the t-th root of
// the slice -- the kernel reads LDS, the host its table.
template <class RootAt>
HD void coset_recover_chain(Fr &pd, Fr &pc, const Fr &xd, const Fr &xc, uint32_t steps, uint32_t valid, RootAt &&root) {
    const Fr one = Fr::one();
    for (uint32_t t = 0; t < steps; t++) {
        const Fr rt = root(t);
        const bool on = t < valid;
        pd = mul(pd, on ? sub(xd, rt) : one);
        pc = mul(pc, on ? sub(xc, rt) : one);
    }
}

}  // namespace ckzg
