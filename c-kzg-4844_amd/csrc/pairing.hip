// pairing.hip -- verify_kzg_proof (src/eip4844/eip4844.c:313-383) for n independent items, one lane per item:
//   * k_point_lhs (k_point_lhs_fr: z, y as device field elements): the left-hand G1 point P1 = C - [y]G + [z]proof of the check
//       e(C - [y]G + [z]proof, [1]_2) * e(-proof, [s]_2) == 1
//     (ckzg_api2.hip: verify_kzg_proof_impl), from the validated points and the 32-byte scalars; an invalid item is
//     replaced by infinity and zero scalars before any arithmetic, so it cannot reach another lane's result
//   * k_pairing_check: that two-pairing check per lane against the line tables of [1]_2 and [s]_2
//     (pairing_dev.hpp on the tower of tower.hpp), one verdict byte per item.
// Host glue: ckzg_api2.hip, verify_point_proofs_on.
#include "device.hpp"
#include "g1_glv_dev.hpp"
#include "pairing_dev.hpp"

namespace ckzg {
namespace dev {

// 32 big-endian bytes -> canonical little-endian limbs; false if the value is not below r (bytes_to_bls_field,
// src/common/bytes.c:106-115)
__device__ __forceinline__ bool fr_raw_from_be32(uint32_t raw[8], const uint8_t *b) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(b);
#pragma unroll
    for (int i = 0; i < 8; i++) raw[i] = __builtin_bswap32(w[7 - i]);
    uint32_t r[8];
    mod_limbs<FrParams>(r);
    return !limbs_geq<8>(raw, r);
}

// pts[0, n) = commitments, pts[n, 2n) = proofs, as decompressed; st_dec / st_sub: their decompression and subgroup
// flags (verify.hip: k_validate_g1<1>, k_subgroup_g1*).  Writes lhs[i] = P1 (XYZZ), neg_proof[i] = -proof (affine) and
// bad[i] = 1 for an invalid item (either point, z or y), whose P1 and -proof are then infinity.
// FR = false: z, y are 32 big-endian bytes each (verify_kzg_proof's arguments).  FR = true: they are field elements as
// the device holds them (the blobs' challenges and evaluations), and unit_bad[i] != 0 marks a blob with an element >= r.
template <bool FR>
__device__ __forceinline__ void point_lhs_lane(G1XYZZ *lhs, G1Affine *neg_proof, uint8_t *bad_out, const G1Affine *pts,
                                               const uint8_t *st_dec, const uint8_t *st_sub, const void *zs, const void *ys,
                                               const uint32_t *unit_bad, size_t n) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const bool live = g < n;
    if (!live) g = n - 1;   // lanes past the end repeat the last item and write nothing
    uint32_t z[8], y[8];
    bool bad;
    if (FR) {
        to_raw<FrParams>(z, static_cast<const Fr *>(zs)[g]);
        to_raw<FrParams>(y, static_cast<const Fr *>(ys)[g]);
        bad = unit_bad[g] != 0;
    } else {
        bad = !fr_raw_from_be32(z, static_cast<const uint8_t *>(zs) + 32 * g);
        bad |= !fr_raw_from_be32(y, static_cast<const uint8_t *>(ys) + 32 * g);
    }
    bad |= (st_dec[g] | st_sub[g] | st_dec[n + g] | st_sub[n + g]) != 0;
    G1Affine c = pts[g], pr = pts[n + g];
    if (bad) {
        c = G1Affine::inf();
        pr = G1Affine::inf();
#pragma unroll
        for (int i = 0; i < 8; i++) z[i] = y[i] = 0;
    }
    uint32_t zg[8], yg[8];
    glv_split(z, zg, zg + 4);
    glv_split(y, yg, yg + 4);
    G1Affine gen;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        gen.x.l[i] = G1_GEN_X[i];
        gen.y.l[i] = G1_GEN_Y[i];
    }
    G1XYZZ acc = xyzz_from_affine(c);
    acc = xyzz_add_ni(acc, glv_half_mul(pr, zg, false));              // [z]proof = [z1]proof + [z2]phi(proof)
    acc = xyzz_add_ni(acc, glv_half_mul(pr, zg + 4, true));
    acc = xyzz_add_ni(acc, xyzz_neg(glv_half_mul(gen, yg, false)));   // - [y]G
    acc = xyzz_add_ni(acc, xyzz_neg(glv_half_mul(gen, yg + 4, true)));
    if (live) {
        lhs[g] = acc;
        neg_proof[g] = affine_neg(pr);   // (infinity stays (0, 0))
        bad_out[g] = bad ? 1 : 0;
    }
}
__global__ __launch_bounds__(64) void k_point_lhs(G1XYZZ *lhs, G1Affine *neg_proof, uint8_t *bad_out, const G1Affine *pts,
                                                  const uint8_t *st_dec, const uint8_t *st_sub, const uint8_t *z32,
                                                  const uint8_t *y32, size_t n) {
    point_lhs_lane<false>(lhs, neg_proof, bad_out, pts, st_dec, st_sub, z32, y32, nullptr, n);
}
__global__ __launch_bounds__(64) void k_point_lhs_fr(G1XYZZ *lhs, G1Affine *neg_proof, uint8_t *bad_out, const G1Affine *pts,
                                                     const uint8_t *st_dec, const uint8_t *st_sub, const Fr *z, const Fr *y,
                                                     const uint32_t *unit_bad, size_t n) {
    point_lhs_lane<true>(lhs, neg_proof, bad_out, pts, st_dec, st_sub, z, y, unit_bad, n);
}

// res[i] = 1 if e(lhs_i, [1]_2) * e(neg_proof_i, [s]_2) == 1, 0 if not, 2 for an invalid item.  tab: the line tables
// lam[68], c[68] of [1]_2, then of [s]_2 (Fp2 entries).  One lane per item, at most one wave per SIMD (an Fp12 is 144
// VGPRs); every lane walks the same table steps.
__global__ __launch_bounds__(64) void k_pairing_check(uint8_t *res, const G1Affine *lhs, const G1Affine *neg_proof,
                                                      const uint8_t *bad, const pdev::Fp2 *__restrict__ tab, size_t n) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const bool live = g < n;
    if (!live) g = n - 1;
    const pdev::LineTable q1 = {tab, tab + pdev::MILLER_STEPS};
    const pdev::LineTable q2 = {tab + 2 * pdev::MILLER_STEPS, tab + 3 * pdev::MILLER_STEPS};
    const bool one = pdev::pairing_product_is_one(lhs[g], q1, neg_proof[g], q2);
    if (live) res[g] = bad[g] ? 2 : (one ? 1 : 0);
}

int point_lhs_enqueue(DeviceCtx *ctx, G1XYZZ *d_lhs, G1Affine *d_neg_proof, uint8_t *d_bad, const G1Affine *d_pts,
                      const uint8_t *d_st_dec, const uint8_t *d_st_sub, const uint8_t *d_z32, const uint8_t *d_y32,
                      size_t n) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_point_lhs, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_lhs, d_neg_proof, d_bad,
                       d_pts, d_st_dec, d_st_sub, d_z32, d_y32, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int point_lhs_fr_enqueue(DeviceCtx *ctx, G1XYZZ *d_lhs, G1Affine *d_neg_proof, uint8_t *d_bad, const G1Affine *d_pts,
                         const uint8_t *d_st_dec, const uint8_t *d_st_sub, const Fr *d_z, const Fr *d_y,
                         const uint32_t *d_unit_bad, size_t n) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_point_lhs_fr, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_lhs, d_neg_proof, d_bad,
                       d_pts, d_st_dec, d_st_sub, d_z, d_y, d_unit_bad, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pairing_check_enqueue(DeviceCtx *ctx, uint8_t *d_res, const G1Affine *d_lhs, const G1Affine *d_neg_proof,
                          const uint8_t *d_bad, const Fp *d_tab, size_t n) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_pairing_check, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_res, d_lhs,
                       d_neg_proof, d_bad, reinterpret_cast<const pdev::Fp2 *>(d_tab), n);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace dev
}  // namespace ckzg
