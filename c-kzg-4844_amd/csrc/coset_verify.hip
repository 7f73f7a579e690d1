// coset_verify.hip -- the device stages of verify_cell_kzg_proof_batch and ckzg_hip_verify_coset_kzg_proof_batch: the
// reference's cell check (eip7594.c:825-974) at every coset size l = 2^e, e = 0 .. 6 (a cell: e = 6), of the 8192-point
// extended domain.  One path for the seven
// sizes: whatever e is, the aggregate has 8192 slots (m = 8192 >> e columns of l), and every kernel maps its lanes over
// the slots, never over the columns, so that a wave is full at e = 0 (8192 columns of one value) as at e = 6 (128
// columns of 64).  The index arithmetic is coset_verify_plan.hpp's; DESIGN.md section 3i.
#include "device.hpp"
#include "rpow2.hpp"
#include "dev_inline.hpp"
#include "fr_lds.hpp"
#include "coset_verify_plan.hpp"

namespace ckzg {
namespace dev {

// Stage 2, per item: r^i in Montgomery form for the aggregation, and in canonical limbs -- plain, and times x_c^l of
// the item's coset -- as the scalars of sum r^i proof_i and sum r^i x_c^l proof_i (eip7594.c:926, :784-812).
__global__ void k_coset_rlc_scalars(Fr *rp, uint32_t *vec_rp, uint32_t *vec_wrp, const uint32_t *coset_idx, const Fr *roots,
                                    RPow2 rp2, uint32_t n, int e) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fr pw = rpow_at(rp2, i);
    rp[i] = pw;
    store_raw(vec_rp + (size_t)i * 8, pw);
    store_raw(vec_wrp + (size_t)i * 8, mul(pw, roots[coset_verify_shift_root(coset_idx[i], e)]));
}

// Stage 2, per distinct commitment: its weight, the sum of r^i over the items that name it (eip7594.c:494-539).  One
// 64-lane workgroup per commitment over its member list.
__global__ __launch_bounds__(64) void k_coset_commit_weights(uint32_t *vec_w, const Fr *rp, const uint32_t *grp_start,
                                                            const uint32_t *members) {
    __shared__ uint32_t sh[8 * 64];
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    Fr acc = Fr::zero();
    for (uint32_t t = grp_start[j] + tid; t < grp_start[j + 1]; t += 64) acc = add(acc, rp[members[t]]);
    lds_st<64>(sh, tid, acc);
    __syncthreads();
    for (uint32_t s2 = 32; s2 >= 1; s2 >>= 1) {
        if (tid < s2) lds_st<64>(sh, tid, add(lds_ld<64>(sh, tid), lds_ld<64>(sh, tid + s2)));
        __syncthreads();
    }
    if (tid == 0) store_raw(vec_w + (size_t)j * 8, lds_ld<64>(sh, 0));
}

// Stage 3: agg[slot(c, j)] = sum over the items i of coset c of r^i y_i[j]  (eip7594.c:661-683).  order[col_start[c] ..
// col_start[c + 1]) lists the items of coset c.  A workgroup takes COSET_AGG_SLOTS_PER_BLOCK consecutive slots, thread
// (slot, p): every parts-th item of the slot's column from the p-th on, then a fold over the parts in LDS.
__global__ void k_coset_aggregate(Fr *agg, const Fr *item_fr, const Fr *rp, const uint32_t *col_start, const uint32_t *order,
                                  uint32_t parts, int e) {
    extern __shared__ uint32_t sh_agg[];   // [parts][8][64]
    constexpr uint32_t S = COSET_AGG_SLOTS_PER_BLOCK;
    const uint32_t lane = threadIdx.x & (S - 1u), p = threadIdx.x / S;
    const uint32_t slot = blockIdx.x * S + lane;
    const uint32_t c = slot >> e, j = slot & ((1u << e) - 1u);
    Fr acc = Fr::zero();
    for (uint32_t t = col_start[c] + p; t < col_start[c + 1]; t += parts) {
        const uint32_t i = order[t];
        acc = add(acc, mul(item_fr[((size_t)i << e) + j], rp[i]));
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
    if (p == 0) agg[slot] = acc;
}

// Stages 4 and 5 in one workgroup of COSET_INTERP_THREADS consecutive slots (whole columns).  Stage 4: the inverse
// transform of each column in LDS -- values in bit-reversed order in, natural coefficients out, e butterfly stages in
// which every lane makes its own output (one product each), times 1 / l; written back in place for whoever wants the
// coefficients of a column.  Stage 5: coefficient k of column c times x_c^-k (eip7594.c:549-566), then a fold over the
// workgroup's columns down to l partial sums, left in partial[block][k].  e = 0: no butterflies, a fold of 256 values.
__global__ __launch_bounds__(COSET_INTERP_THREADS) void k_coset_interp_fold(Fr *partial, Fr *agg, const Fr *roots, Fr inv_l,
                                                                            int e) {
    constexpr uint32_t T = COSET_INTERP_THREADS;
    __shared__ uint32_t sh[8 * T];
    const uint32_t tid = threadIdx.x, slot = blockIdx.x * T + tid;
    const uint32_t l = 1u << e, c = slot >> e, k = slot & (l - 1u);
    Fr v = agg[slot];
    for (int s = 1; s <= e; s++) {
        const uint32_t half = 1u << (s - 1);
        lds_st<T>(sh, tid, v);
        __syncthreads();
        const Fr other = lds_ld<T>(sh, tid ^ half);
        const Fr tw = roots[coset_verify_twiddle_root(k, s)];
        v = (k & half) ? sub(other, mul(v, tw)) : add(v, mul(other, tw));
        __syncthreads();
    }
    v = mul(v, inv_l);
    agg[slot] = v;
    v = mul(v, roots[coset_verify_unshift_root(c, e, k)]);
    lds_st<T>(sh, tid, v);
    __syncthreads();
    for (uint32_t s2 = T >> 1; s2 >= l; s2 >>= 1) {   // tid and tid + s2 hold the same k: s2 is a multiple of l
        if (tid < s2) lds_st<T>(sh, tid, add(lds_ld<T>(sh, tid), lds_ld<T>(sh, tid + s2)));
        __syncthreads();
    }
    if (tid < l) partial[blockIdx.x * l + tid] = lds_ld<T>(sh, tid);
}

// interp[k] = the sum of the COSET_INTERP_BLOCKS partial rows, as canonical limbs: this vector is used as MSM scalars
__global__ void k_coset_interp_final(uint32_t *interp, const Fr *partial, int e) {
    const uint32_t k = threadIdx.x, l = 1u << e;
    if (k >= l) return;
    Fr acc = partial[k];
    for (uint32_t b = 1; b < COSET_INTERP_BLOCKS; b++) acc = add(acc, partial[b * l + k]);
    store_raw(interp + (size_t)k * 8, acc);
}

// The per-item form (ckzg_hip_verify_coset_kzg_proof_batch_locate): what k_cell_interp_digits does
// for 64, at every e.  A 64-lane workgroup takes 64 consecutive slots of the flat value array item_fr[n << e], that is
// 64 >> e whole items: lane t is value t & (l - 1) of item t >> e, and ends with minus coefficient t & (l - 1) of that
// item's interpolation polynomial over its coset, as the signed digits digits[item][w][k] of the fixed-base sum over
// g1_values_monomial[0 .. l - 1].  The e butterfly stages are k_coset_interp_fold's, inside the wave (a lane's partner
// tid ^ half is a value of the same item: half < l); then one product by 1 / l and one by x_c^-k.  e = 0: a lane is an
// item and the coefficient is -y.  Lanes past the last item repeat it and write nothing; an index >= m is clamped for
// the table look-up (k_coset_item_lhs flags the item).  Nothing goes through global memory between values and digits.
__global__ __launch_bounds__(64) void k_coset_item_interp_digits(int16_t *digits, const Fr *item_fr, const uint32_t *coset_idx,
                                                                 const Fr *roots, Fr inv_l, uint32_t n, int e, int wbits, int twin) {
    __shared__ uint32_t sh[8 * 64];
    const uint32_t tid = threadIdx.x, l = 1u << e, k = tid & (l - 1u);
    uint32_t item = blockIdx.x * (64u >> e) + (tid >> e);
    const bool live = item < n;
    if (!live) item = n - 1;
    Fr v = item_fr[((size_t)item << e) + k];
    for (int s = 1; s <= e; s++) {
        const uint32_t half = 1u << (s - 1);
        lds_st<64>(sh, tid, v);
        __syncthreads();
        const Fr other = lds_ld<64>(sh, tid ^ half);
        const Fr tw = roots[coset_verify_twiddle_root(k, s)];
        v = (k & half) ? sub(other, mul(v, tw)) : add(v, mul(other, tw));
        __syncthreads();
    }
    const uint32_t m = coset_verify_cosets(e), c = coset_idx[item] < m ? coset_idx[item] : m - 1u;
    v = neg(mul(mul(v, inv_l), roots[coset_verify_unshift_root(c, e, k)]));
    uint32_t raw[8];
    to_raw<FrParams>(raw, v);
    if (live) glv_digits(digits + ((size_t)item * (size_t)(2 * twin) << e) + k, l, raw, wbits, twin);
}

int coset_item_interp_digits_enqueue(DeviceCtx *ctx, int16_t *d_digits, const Fr *d_item_fr, const uint32_t *d_coset_idx, size_t n,
                                     int e, int wbits, int twin) {
    if (!n) return 0;
    if (e < 0 || e > COSET_MAX_LOG || n > ((size_t)1 << 24)) return 2;
    const size_t per_block = 64u >> e;
    hipLaunchKernelGGL(k_coset_item_interp_digits, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(64), 0, ctx->stream,
                       d_digits, d_item_fr, d_coset_idx, ctx->d_roots, fr_inv_pow2(e), (uint32_t)n, e, wbits, twin);
    HIP_TRY(hipGetLastError());
    return 0;
}

int coset_rlc_scalars_enqueue(DeviceCtx *ctx, Fr *d_rp, uint32_t *d_vec_rp, uint32_t *d_vec_wrp, uint32_t *d_vec_w,
                              const uint32_t *d_coset_idx, const uint32_t *d_grp_start, const uint32_t *d_members, const Fr &r,
                              size_t n, size_t nc, int e) {
    if (!n) return 0;
    if (n >= ((size_t)1 << 24) || e < 0 || e > COSET_MAX_LOG) return 2;
    hipLaunchKernelGGL(k_coset_rlc_scalars, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_rp, d_vec_rp, d_vec_wrp,
                       d_coset_idx, ctx->d_roots, rpow2_of(r), (uint32_t)n, e);
    hipLaunchKernelGGL(k_coset_commit_weights, dim3((unsigned)nc), dim3(64), 0, ctx->stream, d_vec_w, d_rp, d_grp_start, d_members);
    HIP_TRY(hipGetLastError());
    return 0;
}

int coset_aggregate_device(DeviceCtx *ctx, Fr *d_agg, const Fr *d_item_fr, const Fr *d_rp, const uint32_t *d_col_start,
                           const uint32_t *d_order, size_t n_items, int e) {
    if (e < 0 || e > COSET_MAX_LOG) return 2;
    const uint32_t parts = coset_verify_agg_parts(n_items, e);
    hipLaunchKernelGGL(k_coset_aggregate, dim3(COSET_VERIFY_EXT / COSET_AGG_SLOTS_PER_BLOCK), dim3(COSET_AGG_SLOTS_PER_BLOCK * parts),
                       parts > 1 ? parts * COSET_AGG_SLOTS_PER_BLOCK * sizeof(Fr) : 0, ctx->stream, d_agg, d_item_fr, d_rp, d_col_start,
                       d_order, parts, e);
    HIP_TRY(hipGetLastError());
    return 0;
}

int coset_interp_device(DeviceCtx *ctx, uint32_t *d_interp, Fr *d_partial, Fr *d_agg, int e) {
    if (e < 0 || e > COSET_MAX_LOG) return 2;
    hipLaunchKernelGGL(k_coset_interp_fold, dim3(COSET_INTERP_BLOCKS), dim3(COSET_INTERP_THREADS), 0, ctx->stream, d_partial, d_agg,
                       ctx->d_roots, fr_inv_pow2(e), e);
    hipLaunchKernelGGL(k_coset_interp_final, dim3(1), dim3(64), 0, ctx->stream, d_interp, d_partial, e);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace dev
}  // namespace ckzg
