// locate.hip -- the device half of the per-item verdicts at batch cost (ckzg_hip_verify_kzg_proof_batch_locate,
// ckzg_hip_verify_blob_kzg_proof_batch_locate; host glue: ckzg_api2.hip, locate_chunk_from_lhs):
//   * k_locate_scale: per item A_i = [r^i] P1_i and B_i = [r^i] proof_i, the terms of the batch check's two sums
//   * k_g1_scan_tiles / k_g1_scan_offsets: inclusive prefix sums over G1 points (XYZZ, complete addition), which is also
//     what ckzg_hip_g1_prefix_sums exposes on its own.
// With the prefix sums PA, PB on the host, any contiguous range [a, b) of the batch is checked there with two point
// subtractions and one two-pairing check; nothing more is asked of the device.
// The cell form (ckzg_hip_verify_cell_kzg_proof_batch_locate) adds what comes before the scaling:
//   * k_cell_interp_digits: per cell, the coefficients of minus its interpolation polynomial, as the signed digits the
//     fixed-base sum over g1_values_monomial[0..63] reads (k_cell_interp_scale / k_cell_raw_digits: the same in three
//     passes around fr_ntt_batch, the A/B partner)
//   * k_cell_lhs: P1_i = C_i - [I_i(s)]_1 + [h_i^64] proof_i, -proof_i and the item's flag.
// The coset form (ckzg_hip_verify_coset_kzg_proof_batch_locate) is the cell form at every coset
// size: k_coset_item_interp_digits (coset_verify.hip) and k_coset_item_lhs here.
#include "device.hpp"
#include "dev_inline.hpp"
#include "g1_glv_dev.hpp"
#include "rpow2.hpp"
#include "coset_verify_plan.hpp"

namespace ckzg {
namespace dev {

// ab[i] = [r^i] p1[i], ab[n + i] = [r^i] proof_i from neg_proof[i] = -proof_i (both affine, as k_point_lhs and
// batch_to_affine_device leave them; an invalid item is infinity in both and stays so).  Four GLV half-ladders per lane.
__global__ __launch_bounds__(64) void k_locate_scale(G1XYZZ *ab, const G1Affine *p1, const G1Affine *neg_proof, RPow2 rp2,
                                                     uint32_t n) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < n;
    if (!live) g = n - 1;   // lanes past the end repeat the last item and write nothing
    uint32_t k[8], kg[8];
    to_raw<FrParams>(k, rpow_at(rp2, g));
    glv_split(k, kg, kg + 4);
    const G1Affine a = p1[g], np = neg_proof[g];
    const G1XYZZ sa = xyzz_add_ni(glv_half_mul(a, kg, false), glv_half_mul(a, kg + 4, true));
    const G1XYZZ sb = xyzz_add_ni(glv_half_mul(np, kg, false), glv_half_mul(np, kg + 4, true));
    if (live) {
        ab[g] = sa;
        ab[(size_t)n + g] = xyzz_neg(sb);
    }
}

int locate_scale_enqueue(DeviceCtx *ctx, G1XYZZ *d_ab, const G1Affine *d_p1, const G1Affine *d_neg_proof, const Fr &r,
                         size_t n) {
    if (!n) return 0;
    if (n >= ((size_t)1 << 24)) return 2;   // (rpow2.hpp: 24 squarings)
    hipLaunchKernelGGL(k_locate_scale, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_ab, d_p1, d_neg_proof,
                       rpow2_of(r), (uint32_t)n);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the cell form: per-cell interpolation coefficients and left-hand points ----

// (h_c^-1)^k for column c: h_c = w^brp7(c), so the factor is w^((8192 - brp7(c)) k)  (eip7594.c:549-566)
__device__ __forceinline__ Fr cell_coset_inv_pow(const Fr *roots, uint32_t col, uint32_t k) {
    const uint32_t rb = __brev(col) >> 25;   // the low seven bits of the column, reversed (an index >= 128 is flagged elsewhere)
    return roots[((8192u - rb) * k) & 8191u];
}

// One wave per cell: lane t holds field element t of the cell (bit-reversed order, as a cell is stored) and ends with
// minus coefficient t of the cell's interpolation polynomial over its coset, as k_fk20_digits-style signed digits
// digits[cell][w][t].  The 64-point inverse transform is fr_ntt_batch(.., 6, false, true, true) inside the wave: six
// DIT stages, each one twiddle product on the upper lane of a pair and one exchange through LDS (limb-major, so the 64
// lanes fall on 64 banks); then one product by 1/64 and one by (h^-1)^t.  Nothing goes through global memory between
// the cell's field elements and its digits.
__global__ __launch_bounds__(64) void k_cell_interp_digits(int16_t *digits, const Fr *cell_fr, const uint32_t *col,
                                                           const Fr *roots, Fr inv64, int wbits, int twin) {
    __shared__ uint32_t sh[8][64];
    const size_t cell = blockIdx.x;
    const uint32_t t = threadIdx.x;
    Fr v = cell_fr[cell * 64 + t];
#pragma unroll 1
    for (int s = 1; s <= 6; s++) {
        const uint32_t half = 1u << (s - 1), j = t & (half - 1);
        const bool upper = (t & half) != 0;
        if (upper && j) v = mul(v, roots[N_EXT - j * (N_EXT >> s)]);
#pragma unroll
        for (int k = 0; k < 8; k++) sh[k][t] = v.l[k];
        __syncthreads();
        Fr o;
#pragma unroll
        for (int k = 0; k < 8; k++) o.l[k] = sh[k][t ^ half];
        __syncthreads();
        v = upper ? sub(o, v) : add(v, o);
    }
    v = neg(mul(mul(v, inv64), cell_coset_inv_pow(roots, col[cell], t)));
    uint32_t raw[8];
    to_raw<FrParams>(raw, v);
    glv_digits(digits + cell * (size_t)(2 * twin) * 64 + t, 64, raw, wbits, twin);
}

// The three-pass form, after fr_ntt_batch over the cells: coefficient g -> minus itself times (h^-1)^k, canonical limbs
__global__ void k_cell_interp_scale(uint32_t *raw_out, const Fr *coef, const uint32_t *col, const Fr *roots, size_t total) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= total) return;
    uint32_t raw[8];
    to_raw<FrParams>(raw, neg(mul(coef[g], cell_coset_inv_pow(roots, col[g >> 6], (uint32_t)g & 63u))));
#pragma unroll
    for (int k = 0; k < 8; k++) raw_out[g * 8 + k] = raw[k];
}
// ... and its digits, digits[cell][w][k]
__global__ void k_cell_raw_digits(int16_t *digits, const uint32_t *raw_in, size_t total, int wbits, int twin) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= total) return;
    uint32_t raw[8];
#pragma unroll
    for (int k = 0; k < 8; k++) raw[k] = raw_in[g * 8 + k];
    glv_digits(digits + (g >> 6) * (size_t)(2 * twin) * 64 + (g & 63), 64, raw, wbits, twin);
}

int cell_interp_digits_enqueue(DeviceCtx *ctx, int16_t *d_digits, Fr *d_cell_fr, const uint32_t *d_col, size_t n, int wbits,
                               int twin, bool fused, uint32_t *d_raw_tmp) {
    if (!n) return 0;
    if (n > 0x7fffffffu) return 2;
    if (fused) {
        hipLaunchKernelGGL(k_cell_interp_digits, dim3((unsigned)n), dim3(64), 0, ctx->stream, d_digits, d_cell_fr, d_col,
                           ctx->d_roots, fr_inv_pow2(6), wbits, twin);
    } else {
        // whole tiles of 4096 elements: d_cell_fr has room for the cells up to the next multiple of 64
        if (int rc = fr_ntt_batch(ctx, d_cell_fr, (n + 63) / 64 * 64, 6, false, true, true)) return rc;
        const size_t total = n * 64;
        hipLaunchKernelGGL(k_cell_interp_scale, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_raw_tmp,
                           d_cell_fr, d_col, ctx->d_roots, total);
        hipLaunchKernelGGL(k_cell_raw_digits, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_digits,
                           d_raw_tmp, total, wbits, twin);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// pts[0, n) = proofs, pts[n, n + nc) = the chunk's distinct commitments, as decompressed; st_dec / st_sub: their
// n + nc decompression and subgroup flags.  Item g names commitment commit[g] and column col[g]; cell_bad[g] != 0 marks
// a cell with a field element >= r; minus_interp[g] = -[I_g(s)]_1.  Writes lhs[g] = P1_g (XYZZ), neg_proof[g] = -proof_g
// (affine) and bad[g] = 1 for an invalid item (column >= 128, cell, commitment or proof), whose P1 and -proof are then
// infinity.  [h^64] proof is one GLV ladder per lane, h^64 = w^(64 brp7(column)).
__global__ __launch_bounds__(64) void k_cell_lhs(G1XYZZ *lhs, G1Affine *neg_proof, uint8_t *bad_out, const G1Affine *pts,
                                                 const uint8_t *st_dec, const uint8_t *st_sub, const G1XYZZ *minus_interp,
                                                 const uint32_t *col, const uint32_t *commit, const uint32_t *cell_bad,
                                                 const Fr *roots, size_t n) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const bool live = g < n;
    if (!live) g = n - 1;   // lanes past the end repeat the last item and write nothing
    const size_t cg = n + commit[g];
    const uint32_t c7 = col[g];
    const bool bad = c7 >= 128u || cell_bad[g] != 0 || (st_dec[g] | st_sub[g] | st_dec[cg] | st_sub[cg]) != 0;
    G1Affine c = pts[cg], pr = pts[g];
    G1XYZZ mi = minus_interp[g];
    if (bad) {
        c = G1Affine::inf();
        pr = G1Affine::inf();
        mi = G1XYZZ::inf();
    }
    uint32_t h[8], hg[8];
    to_raw<FrParams>(h, roots[(size_t)(__brev(c7) >> 25) * N_CELL]);
    glv_split(h, hg, hg + 4);
    G1XYZZ acc = xyzz_add_ni(xyzz_from_affine(c), mi);
    acc = xyzz_add_ni(acc, glv_half_mul(pr, hg, false));   // [h^64]proof = [h1]proof + [h2]phi(proof)
    acc = xyzz_add_ni(acc, glv_half_mul(pr, hg + 4, true));
    if (live) {
        lhs[g] = acc;
        neg_proof[g] = affine_neg(pr);   // (infinity stays (0, 0))
        bad_out[g] = bad ? 1 : 0;
    }
}

int cell_lhs_enqueue(DeviceCtx *ctx, G1XYZZ *d_lhs, G1Affine *d_neg_proof, uint8_t *d_bad, const G1Affine *d_pts,
                     const uint8_t *d_st_dec, const uint8_t *d_st_sub, const G1XYZZ *d_minus_interp, const uint32_t *d_col,
                     const uint32_t *d_commit, const uint32_t *d_cell_bad, size_t n) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_cell_lhs, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_lhs, d_neg_proof, d_bad, d_pts,
                       d_st_dec, d_st_sub, d_minus_interp, d_col, d_commit, d_cell_bad, ctx->d_roots, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the coset form: k_cell_lhs with the coset size a parameter (ckzg_hip_verify_coset_kzg_proof_batch_locate) ----

// As k_cell_lhs, for cosets of l = 2^e values: item g names coset idx[g] of the m = 8192 >> e; val_bad[g] != 0 marks an
// item with a value >= r.  P1_g = C_g + (-[I_g(s)]_1) + [x_c^l] proof_g, x_c^l = roots[coset_verify_shift_root(c, e)].
// An index >= m makes the item invalid; it is clamped for the look-up only.
__global__ __launch_bounds__(64) void k_coset_item_lhs(G1XYZZ *lhs, G1Affine *neg_proof, uint8_t *bad_out, const G1Affine *pts,
                                                       const uint8_t *st_dec, const uint8_t *st_sub, const G1XYZZ *minus_interp,
                                                       const uint32_t *idx, const uint32_t *commit, const uint32_t *val_bad,
                                                       const Fr *roots, size_t n, int e) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const bool live = g < n;
    if (!live) g = n - 1;   // lanes past the end repeat the last item and write nothing
    const size_t cg = n + commit[g];
    const uint32_t m = coset_verify_cosets(e), ci = idx[g];
    const bool bad = ci >= m || val_bad[g] != 0 || (st_dec[g] | st_sub[g] | st_dec[cg] | st_sub[cg]) != 0;
    G1Affine c = pts[cg], pr = pts[g];
    G1XYZZ mi = minus_interp[g];
    if (bad) {
        c = G1Affine::inf();
        pr = G1Affine::inf();
        mi = G1XYZZ::inf();
    }
    uint32_t h[8], hg[8];
    to_raw<FrParams>(h, roots[coset_verify_shift_root(ci < m ? ci : m - 1u, e)]);
    glv_split(h, hg, hg + 4);
    G1XYZZ acc = xyzz_add_ni(xyzz_from_affine(c), mi);
    acc = xyzz_add_ni(acc, glv_half_mul(pr, hg, false));   // [x_c^l]proof = [h1]proof + [h2]phi(proof)
    acc = xyzz_add_ni(acc, glv_half_mul(pr, hg + 4, true));
    if (live) {
        lhs[g] = acc;
        neg_proof[g] = affine_neg(pr);   // (infinity stays (0, 0))
        bad_out[g] = bad ? 1 : 0;
    }
}

int coset_item_lhs_enqueue(DeviceCtx *ctx, G1XYZZ *d_lhs, G1Affine *d_neg_proof, uint8_t *d_bad, const G1Affine *d_pts,
                           const uint8_t *d_st_dec, const uint8_t *d_st_sub, const G1XYZZ *d_minus_interp, const uint32_t *d_idx,
                           const uint32_t *d_commit, const uint32_t *d_val_bad, size_t n, int e) {
    if (!n) return 0;
    if (e < 0 || e > COSET_MAX_LOG) return 2;
    hipLaunchKernelGGL(k_coset_item_lhs, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_lhs, d_neg_proof, d_bad,
                       d_pts, d_st_dec, d_st_sub, d_minus_interp, d_idx, d_commit, d_val_bad, ctx->d_roots, n, e);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- inclusive prefix sums over G1 ----
// One workgroup scans a tile of SCAN_TILE points through LDS (Hillis-Steele: log2(SCAN_TILE) rounds of one complete
// addition per lane; a point is 48 words, kept word-major so that a wave's accesses fall on distinct banks: 48 KB) and
// leaves the tile's total; the totals are scanned the same way, recursively, and every tile but the first then adds the
// sum of the tiles before it.  About ten additions per point.  nseg independent arrays of n points each go in one
// launch (blockIdx.y): the A and the B points of a chunk.
constexpr int SCAN_TILE = 256;
constexpr int XYZZ_WORDS = sizeof(G1XYZZ) / 4;
static_assert(XYZZ_WORDS == 48, "G1XYZZ is four Fp of twelve words");

__global__ __launch_bounds__(SCAN_TILE) void k_g1_scan_tiles(G1XYZZ *data, G1XYZZ *totals, size_t n, size_t ntiles) {
    __shared__ uint32_t sh[XYZZ_WORDS][SCAN_TILE];
    G1XYZZ *d = data + blockIdx.y * n;
    const uint32_t t = threadIdx.x;
    const size_t g = blockIdx.x * (size_t)SCAN_TILE + t;
    G1XYZZ own = g < n ? d[g] : G1XYZZ::inf();   // past the end: the identity, so the last lane ends with the tile's total
    uint32_t *w = reinterpret_cast<uint32_t *>(&own);
#pragma unroll 1
    for (uint32_t off = 1; off < SCAN_TILE; off <<= 1) {
#pragma unroll
        for (int j = 0; j < XYZZ_WORDS; j++) sh[j][t] = w[j];
        __syncthreads();
        if (t >= off) {
            G1XYZZ left;
            uint32_t *lw = reinterpret_cast<uint32_t *>(&left);
#pragma unroll
            for (int j = 0; j < XYZZ_WORDS; j++) lw[j] = sh[j][t - off];
            own = xyzz_add_ni(left, own);
        }
        __syncthreads();
    }
    if (g < n) d[g] = own;
    if (t == SCAN_TILE - 1) totals[blockIdx.y * ntiles + blockIdx.x] = own;
}

// data[tile b][*] += offsets[b - 1] for every tile b >= 1 (offsets: the scanned totals of the tiles)
__global__ __launch_bounds__(SCAN_TILE) void k_g1_scan_offsets(G1XYZZ *data, const G1XYZZ *offsets, size_t n, size_t ntiles) {
    const size_t b = (size_t)blockIdx.x + 1, g = b * SCAN_TILE + threadIdx.x;
    if (g >= n) return;
    G1XYZZ *d = data + blockIdx.y * n;
    d[g] = xyzz_add_ni(offsets[blockIdx.y * ntiles + b - 1], d[g]);
}

size_t g1_prefix_scan_scratch_points(size_t n, size_t nseg) {
    size_t pts = 0;
    do {   // one total per tile, level by level until a level is one tile
        n = (n + SCAN_TILE - 1) / SCAN_TILE;
        pts += n * nseg;
    } while (n > 1);
    return pts;
}

int g1_prefix_scan_enqueue(DeviceCtx *ctx, G1XYZZ *d_data, G1XYZZ *d_scratch, size_t n, size_t nseg) {
    if (!n || !nseg) return 0;
    const size_t ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (ntiles > 0x7fffffffu || nseg > 65535) return 2;
    hipLaunchKernelGGL(k_g1_scan_tiles, dim3((unsigned)ntiles, (unsigned)nseg), dim3(SCAN_TILE), 0, ctx->stream, d_data,
                       d_scratch, n, ntiles);
    HIP_TRY(hipGetLastError());
    if (ntiles == 1) return 0;
    // the tiles' totals: nseg arrays of ntiles points, scanned in place behind their own scratch
    if (int rc = g1_prefix_scan_enqueue(ctx, d_scratch, d_scratch + ntiles * nseg, ntiles, nseg)) return rc;
    hipLaunchKernelGGL(k_g1_scan_offsets, dim3((unsigned)(ntiles - 1), (unsigned)nseg), dim3(SCAN_TILE), 0, ctx->stream,
                       d_data, d_scratch, n, ntiles);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace dev
}  // namespace ckzg
