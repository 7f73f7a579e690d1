// coset_groups.hip -- the device stages of ckzg_hip_verify_coset_kzg_proof_batch_groups: the check of coset_verify.hip
// at every coset size l = 2^e, e = 0 .. 6, once per chunk of groups, segmented by group.  The index maps and the launch
// pickers are the host's (coset_groups_plan.hpp); gd is its group table
// start[G + 1] | first term of A_g [G] | distinct commitments of g [G] | first term of B_g [G], and sc the scalar
// vector of all jobs (canonical limbs, 8 words per term, zero where a term is padding).  A row is a distinct
// (group, coset) pair: l values; the R rows of a chunk lie back to back, the rows of a group together.  As in
// coset_verify.hip every kernel maps its lanes over slots -- items, the R l row slots, the G l outputs -- never over
// rows, cosets or groups, so that a wave is as full at e = 0 as at e = 6.  DESIGN.md section 3i.2.
#include "device.hpp"
#include "dev_inline.hpp"
#include "fr_lds.hpp"
#include "coset_groups_plan.hpp"

namespace ckzg {
namespace dev {

// Item i of group g gets r_g^(i - start_g) by square-and-multiply from its offset (<= 2 log2 of the group's size
// products, no lane waits for another): in Montgomery form for the aggregation, in canonical limbs on the item's proof in B_g, and times x_c^l of its coset
// on the same proof in A_g.
__global__ void k_coset_group_rlc_scalars(Fr *rp, uint32_t *sc, const uint32_t *item_grp, const uint32_t *item_col,
                                          const uint32_t *gd, const Fr *r, const Fr *roots, uint32_t n, uint32_t ngroups, int e) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = item_grp[i], off = i - gd[g];
    Fr base = r[g], pw = Fr::one();
#pragma unroll 1
    for (uint32_t x = off; x; x >>= 1) {
        if (x & 1u) pw = mul(pw, base);
        base = mul(base, base);
    }
    rp[i] = pw;
    const size_t ta = (size_t)gd[ngroups + 1 + g] + gd[2 * ngroups + 1 + g] + off, tb = (size_t)gd[3 * ngroups + 1 + g] + off;
    store_raw(sc + ta * 8, mul(pw, roots[coset_verify_shift_root(item_col[i], e)]));
    store_raw(sc + tb * 8, pw);
}

// rows[slot(t, j)] = sum over the items i of row t of r^i y_i[j]: k_coset_aggregate with the chunk's rows in the place
// of the m cosets.  order[row_start[t] .. row_start[t + 1]) lists the items of row t.  A workgroup takes
// COSET_AGG_SLOTS_PER_BLOCK consecutive slots of the nslots = R l, thread (slot, p): every parts-th item of the slot's
// row from the p-th on, then a fold over the parts in LDS.  A lane past the last slot adds nothing and writes nothing.
__global__ void k_coset_group_aggregate(Fr *rows, const Fr *item_fr, const Fr *rp, const uint32_t *row_start, const uint32_t *order,
                                        uint32_t nslots, uint32_t parts, int e) {
    extern __shared__ uint32_t sh_agg[];   // [parts][8][64]
    constexpr uint32_t S = COSET_AGG_SLOTS_PER_BLOCK;
    const uint32_t lane = threadIdx.x & (S - 1u), p = threadIdx.x / S;
    const uint32_t slot = blockIdx.x * S + lane;
    const bool live = slot < nslots;
    const uint32_t t = slot >> e, j = slot & ((1u << e) - 1u);
    Fr acc = Fr::zero();
    if (live) {
        for (uint32_t q = row_start[t] + p; q < row_start[t + 1]; q += parts) {
            const uint32_t i = order[q];
            acc = add(acc, mul(item_fr[((size_t)i << e) + j], rp[i]));
        }
    }
    if (parts > 1) {
        lds_st<S>(sh_agg + p * 8 * S, lane, acc);
        __syncthreads();
        for (uint32_t s2 = parts >> 1; s2 >= 1; s2 >>= 1) {
            if (p < s2) lds_st<S>(sh_agg + p * 8 * S, lane, add(lds_ld<S>(sh_agg + p * 8 * S, lane), lds_ld<S>(sh_agg + (p + s2) * 8 * S, lane)));
            __syncthreads();
        }
        acc = lds_ld<S>(sh_agg, lane);
    }
    if (p == 0 && live) rows[slot] = acc;
}

// Each row's interpolation polynomial over its coset, in place: a workgroup takes COSET_INTERP_THREADS consecutive row
// slots (whole rows) and runs the e butterfly stages of k_coset_interp_fold in LDS -- values in bit-reversed order in,
// natural coefficients out, every lane its own output -- then one product by 1 / l and one by x_c^-k, c the row's
// coset.  No fold here: the rows of a group are added by k_coset_group_interp_sum.  A lane past the last slot works on
// zero and writes nothing; its partner tid ^ half is a slot of the same row, so live lanes never read it.
__global__ __launch_bounds__(COSET_INTERP_THREADS) void k_coset_group_interp(Fr *rows, const uint32_t *row_col, const Fr *roots,
                                                                             Fr inv_l, uint32_t nslots, int e) {
    constexpr uint32_t T = COSET_INTERP_THREADS;
    __shared__ uint32_t sh[8 * T];
    const uint32_t tid = threadIdx.x, slot = blockIdx.x * T + tid;
    const bool live = slot < nslots;
    const uint32_t l = 1u << e, k = slot & (l - 1u);
    Fr v = live ? rows[slot] : Fr::zero();
    for (int s = 1; s <= e; s++) {
        const uint32_t half = 1u << (s - 1);
        lds_st<T>(sh, tid, v);
        __syncthreads();
        const Fr other = lds_ld<T>(sh, tid ^ half);
        const Fr tw = roots[coset_verify_twiddle_root(k, s)];
        v = (k & half) ? sub(other, mul(v, tw)) : add(v, mul(other, tw));
        __syncthreads();
    }
    if (live) rows[slot] = mul(mul(v, inv_l), roots[coset_verify_unshift_root(row_col[slot >> e], e, k)]);
}

// -interp_g[k] = -sum over the rows of group g of their k-th term (k_coset_group_interp has taken the coset factors
// out), in canonical limbs onto the k-th setup point of A_g: the interpolation commitment is subtracted by its scalars.
// One lane per (output, part) over the nout = G l outputs, COSET_GROUPS_SUM_OUT_PER_BLOCK outputs a workgroup: every
// parts-th row of the group from the p-th on, then a fold over the parts in LDS.  An empty group has no such term.
__global__ void k_coset_group_interp_sum(uint32_t *sc, const Fr *rows, const uint32_t *grp_rows, const uint32_t *gd, uint32_t nout,
                                         uint32_t ngroups, uint32_t parts, int e) {
    extern __shared__ uint32_t sh_sum[];   // [parts][8][64]
    constexpr uint32_t S = COSET_GROUPS_SUM_OUT_PER_BLOCK;
    const uint32_t lane = threadIdx.x & (S - 1u), p = threadIdx.x / S;
    const uint32_t o = blockIdx.x * S + lane;
    const bool live = o < nout;
    const uint32_t g = live ? o >> e : 0u, k = o & ((1u << e) - 1u);
    Fr acc = Fr::zero();
    if (live) {
        for (uint32_t t = grp_rows[g] + p; t < grp_rows[g + 1]; t += parts) acc = add(acc, rows[((size_t)t << e) + k]);
    }
    if (parts > 1) {
        lds_st<S>(sh_sum + p * 8 * S, lane, acc);
        __syncthreads();
        for (uint32_t s2 = parts >> 1; s2 >= 1; s2 >>= 1) {
            if (p < s2) lds_st<S>(sh_sum + p * 8 * S, lane, add(lds_ld<S>(sh_sum + p * 8 * S, lane), lds_ld<S>(sh_sum + (p + s2) * 8 * S, lane)));
            __syncthreads();
        }
        acc = lds_ld<S>(sh_sum, lane);
    }
    const uint32_t n = gd[g + 1] - gd[g];
    if (p == 0 && live && n != 0) {
        const size_t t = (size_t)gd[ngroups + 1 + g] + gd[2 * ngroups + 1 + g] + n + k;
        store_raw(sc + t * 8, neg(acc));
    }
}

int coset_group_rlc_scalars_enqueue(DeviceCtx *ctx, Fr *d_rp, uint32_t *d_sc, const uint32_t *d_item_grp, const uint32_t *d_item_col,
                                    const uint32_t *d_gd, const Fr *d_r, const uint32_t *d_pair_start, const uint32_t *d_pair_members,
                                    const uint32_t *d_pair_term, size_t n, size_t ngroups, size_t npairs, int e) {
    if (!n) return 0;
    if (n >= ((size_t)1 << 31) || e < 0 || e > COSET_MAX_LOG) return 2;
    hipLaunchKernelGGL(k_coset_group_rlc_scalars, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_rp, d_sc, d_item_grp,
                       d_item_col, d_gd, d_r, ctx->d_roots, (uint32_t)n, (uint32_t)ngroups, e);
    HIP_TRY(hipGetLastError());
    return group_commit_weights_enqueue(ctx, d_sc, d_rp, d_pair_start, d_pair_members, d_pair_term, npairs);
}

int coset_group_aggregate_device(DeviceCtx *ctx, Fr *d_rows, const Fr *d_item_fr, const Fr *d_rp, const uint32_t *d_row_start,
                                 const uint32_t *d_row_order, size_t n_items, size_t nrows, int e) {
    if (!nrows) return 0;
    if (e < 0 || e > COSET_MAX_LOG || (nrows << e) >= ((size_t)1 << 31)) return 2;
    const uint32_t parts = coset_groups_agg_parts(n_items, nrows);
    hipLaunchKernelGGL(k_coset_group_aggregate, dim3((unsigned)coset_groups_agg_blocks(nrows, e)), dim3(COSET_AGG_SLOTS_PER_BLOCK * parts),
                       parts > 1 ? parts * COSET_AGG_SLOTS_PER_BLOCK * sizeof(Fr) : 0, ctx->stream, d_rows, d_item_fr, d_rp, d_row_start,
                       d_row_order, (uint32_t)(nrows << e), parts, e);
    HIP_TRY(hipGetLastError());
    return 0;
}

int coset_group_interp_device(DeviceCtx *ctx, Fr *d_rows, const uint32_t *d_row_col, size_t nrows, int e) {
    if (!nrows) return 0;
    if (e < 0 || e > COSET_MAX_LOG || (nrows << e) >= ((size_t)1 << 31)) return 2;
    hipLaunchKernelGGL(k_coset_group_interp, dim3((unsigned)coset_groups_interp_blocks(nrows, e)), dim3(COSET_INTERP_THREADS), 0,
                       ctx->stream, d_rows, d_row_col, ctx->d_roots, fr_inv_pow2(e), (uint32_t)(nrows << e), e);
    HIP_TRY(hipGetLastError());
    return 0;
}

int coset_group_interp_sum_device(DeviceCtx *ctx, uint32_t *d_sc, const Fr *d_rows, const uint32_t *d_grp_rows, const uint32_t *d_gd,
                                  size_t nrows, size_t ngroups, int e) {
    if (!ngroups) return 0;
    if (e < 0 || e > COSET_MAX_LOG || (ngroups << e) >= ((size_t)1 << 31)) return 2;
    const uint32_t parts = coset_groups_sum_parts(nrows, ngroups);
    hipLaunchKernelGGL(k_coset_group_interp_sum, dim3((unsigned)coset_groups_sum_blocks(ngroups, e)),
                       dim3(COSET_GROUPS_SUM_OUT_PER_BLOCK * parts), parts > 1 ? parts * COSET_GROUPS_SUM_OUT_PER_BLOCK * sizeof(Fr) : 0,
                       ctx->stream, d_sc, d_rows, d_grp_rows, d_gd, (uint32_t)(ngroups << e), (uint32_t)ngroups, parts, e);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace dev
}  // namespace ckzg
