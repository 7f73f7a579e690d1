// coset_repair.hip -- the device stages of the checks that ckzg_hip_repair_cosets_and_kzg_proofs_rows adds to the
// recovery pipeline (ckzg_api2.hip: recover_chunks with a RecoverChecks): the degree flag of a row's coefficients, the
// scalar recoding of a row's blob half straight from the pipeline's Fr rows (then the commitment MSM of msm.hip), and
// the comparison of the commitments with the ones the caller gave.  Planning: coset_repair_plan.hpp; DESIGN.md section 3k.
#include "device.hpp"
#include "dev_inline.hpp"

namespace ckzg {
namespace dev {

namespace {

constexpr uint32_t ROW = 8192, HALF = 4096;   // values of a row; of its blob half = coefficients below the degree bound
constexpr uint32_t HD_THREADS = 1024;          // k_rows_high_degree: 16 waves a row, 8 loads of 16 bytes a lane

__device__ __forceinline__ Fr vld_fr(const Fr *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    uint4 a = q[0], b = q[1];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

// flags[row] = 1 if any of the coefficients 4096 .. 8191 of rows[row][0 .. 8191] is not zero, else 0.
// The comparison is one of field elements: an Fr is Mont<FrParams>, "fully reduced: 0 <= value < m" (field.hpp), and
// the values here are what k_fr_mul_inplace stored, the result of mul(), whose last step is the conditional
// subtraction of the modulus.  0 * R mod r = 0, so zero is the all-zero limb pattern and nothing else is: the test is
// an OR over the words.  One workgroup per row reads the row's upper 128 KB once: lane t of the workgroup takes the
// uint4 at t, t + 1024, ... (a wave reads 1 KB contiguous per load, eight independent loads in flight per lane).
// Every row's flag is written, by a plain vector store of lane 0: the flags need no reset.
__global__ __launch_bounds__(HD_THREADS) void k_rows_high_degree(uint32_t *flags, const Fr *rows) {
    __shared__ uint32_t sh[HD_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    const uint4 *p = reinterpret_cast<const uint4 *>(rows + (size_t)blockIdx.x * ROW + HALF);
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t j = 0; j < HALF * 2 / HD_THREADS; j++) {
        const uint4 v = p[j * HD_THREADS + tid];
        acc |= v.x | v.y | v.z | v.w;
    }
    const bool any = __ballot(acc != 0) != 0;
    if ((tid & 63) == 0) sh[tid >> 6] = any ? 1u : 0u;
    __syncthreads();
    if (tid == 0) {
        uint32_t r = 0;
#pragma unroll
        for (uint32_t w = 0; w < HD_THREADS / 64; w++) r |= sh[w];
        flags[blockIdx.x] = r;
    }
}

// The recoding of k_blob_digits (msm.hip) for scalars the pipeline already holds: one thread per value i < 4096 of a
// row, read as Montgomery Fr at rows[row][i] (row stride 8192: the second half of a row is never touched), taken out of
// Montgomery form and split into the signed GLV digits digits[row][w][i] that k_msm_accumulate reads.  The values are
// canonical (see above), so there is no range flag.
__global__ void k_fr_rows_digits(int16_t *digits, const Fr *rows, size_t total, int wbits, int twin) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const size_t row = gid >> 12;
    const uint32_t i = (uint32_t)(gid & (HALF - 1));
    uint32_t s[8];
    to_raw<FrParams>(s, vld_fr(rows + row * ROW + i));
    glv_digits(digits + row * (size_t)(2 * twin) * N_BLOB + i, N_BLOB, s, wbits, twin);
}

// flags[row] = 1 if the 48 bytes got[row] and want[row] differ, else 0 (both 16-byte aligned: 48-byte rows of
// 256-byte aligned buffers).  Every row's flag is written.
__global__ void k_commit_compare(uint32_t *flags, const uint4 *got, const uint4 *want, uint32_t nrows) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t j = 0; j < 3; j++) {
        const uint4 a = got[3 * (size_t)row + j], b = want[3 * (size_t)row + j];
        acc |= (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w);
    }
    flags[row] = acc ? 1u : 0u;
}

int rows_high_degree_enqueue(DeviceCtx *ctx, uint32_t *d_flags, const Fr *d_rows, size_t nrows) {
    if (!nrows) return 0;
    if (nrows > 0x7fffffffu) return 2;
    hipLaunchKernelGGL(k_rows_high_degree, dim3((unsigned)nrows), dim3(HD_THREADS), 0, ctx->stream, d_flags, d_rows);
    HIP_TRY(hipGetLastError());
    return 0;
}

// digits + partial sums in ctx->scratch, which must hold commit_scratch_bytes(ctx, nrows) (the caller reserves: a
// reservation may wait for the stream); enqueue-only
int fr_rows_commit_enqueue(DeviceCtx *ctx, uint8_t *d_out48, const Fr *d_rows, size_t nrows) {
    if (!nrows) return 0;
    const FixedBaseTable &t = ctx->commit;
    if (!t.d_table || t.npoints != N_BLOB || nrows > (0x7fffffffu >> 12)) return 2;
    const size_t dig_bytes = align_up(nrows * (size_t)t.nwin * t.npoints * sizeof(int16_t), 256);
    if (ctx->scratch.cap < commit_scratch_bytes(ctx, nrows) ||
        ctx->scratch.cap < dig_bytes + msm_partials_needed(t, nrows) * sizeof(G1XYZZ))
        return 2;
    uint8_t *base = static_cast<uint8_t *>(ctx->scratch.ptr);
    int16_t *d_digits = reinterpret_cast<int16_t *>(base);
    G1XYZZ *d_partials = reinterpret_cast<G1XYZZ *>(base + dig_bytes);
    const size_t total = nrows * HALF;
    hipLaunchKernelGGL(k_fr_rows_digits, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_digits, d_rows,
                       total, t.wbits, t.twin);
    HIP_TRY(hipGetLastError());
    return msm_from_digits_device(ctx, t, d_out48, d_digits, d_partials, nrows);
}

int commit_compare_enqueue(DeviceCtx *ctx, uint32_t *d_flags, const uint8_t *d_got48, const uint8_t *d_want48, size_t nrows) {
    if (!nrows) return 0;
    if (nrows > 0x7fffffffu || ((uintptr_t)d_got48 | (uintptr_t)d_want48) % 16) return 2;
    hipLaunchKernelGGL(k_commit_compare, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, ctx->stream, d_flags,
                       reinterpret_cast<const uint4 *>(d_got48), reinterpret_cast<const uint4 *>(d_want48), (uint32_t)nrows);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace dev
}  // namespace ckzg
