// coset_recover.hip -- the device stages of ckzg_hip_recover_cosets_and_kzg_proofs_rows that depend on the coset size
// l = 2^e, e = 0 .. 6: Z over the domain and 1 / Z over the shifted coset of every distinct set of missing cosets, the
// per-coset multiplication, and the scatter of the held cosets into the zeroed row image.  Index maps and the launch
// decisions: coset_recover_plan.hpp; arithmetic: coset_recover_factors.hpp; DESIGN.md section 3j.
#include "device.hpp"
#include "dev_inline.hpp"
#include "fr_inv.hpp"
#include "coset_recover_plan.hpp"
#include "coset_recover_factors.hpp"

namespace ckzg {
namespace dev {

namespace {

constexpr uint32_t T = COSET_RECOVER_THREADS;

__device__ __forceinline__ Fr vld_fr(const Fr *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    uint4 a = q[0], b = q[1];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}

__device__ __forceinline__ void vst_fr(Fr *p, const Fr &v) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

__device__ __noinline__ Fr fr_inv_dev(const Fr &a) { return fr_inv_safegcd(a); }

// An Fr vector in LDS, limb-major (limb k of element i at sh[k * T + i]): lanes that read consecutive elements read
// consecutive words
__device__ __forceinline__ Fr lds_ld(const uint32_t *sh, uint32_t i) {
    Fr r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = sh[k * T + i];
    return r;
}
__device__ __forceinline__ void lds_st(uint32_t *sh, uint32_t i, const Fr &v) {
#pragma unroll
    for (int k = 0; k < 8; k++) sh[k * T + i] = v.l[k];
}

}  // namespace

// z_domain[s][c], z_coset_inv[s][c] for every distinct set s of a chunk and every coset c < m = 8192 >> e.
// A workgroup of blockDim.x = coset_recover_block(e, parts) lanes belongs to ONE set and holds every part of
// cpw = blockDim.x / parts consecutive cosets: lane = part * cpw + (coset - first), so that a wave is one part
// wherever cpw >= 64 and its lanes read one root per step.  The slices have len = ceil(count / parts) steps each, a
// trip count that is uniform over the workgroup; the steps past a slice's end multiply by 1 (no branch).  The roots are
// gathers of 32 B from d_roots through the missing list, and every lane of a part reads the same ones: per tile of cpw
// steps each lane fetches ONE root (parts * cpw = blockDim.x of them, 8 KB) into LDS and the chains read them there.
// The partial products are folded over the parts in LDS (16 KB), and the lanes of part 0 invert the coset value.
// 24 KB of LDS a workgroup: six workgroups fit a CU's 160 KB, more than its SIMDs take at this register count.
__global__ __launch_bounds__(COSET_RECOVER_THREADS) void k_coset_recover_factors(Fr *z_domain, Fr *z_coset_inv,
                                                                                 const uint32_t *miss,
                                                                                 const uint32_t *miss_start, const Fr *roots,
                                                                                 const Fr *shift, int e, uint32_t parts) {
    __shared__ uint32_t sh_r[8 * T], sh_d[8 * T], sh_c[8 * T];
    const uint32_t tid = threadIdx.x, m = COSET_RECOVER_EXT >> e, cpw = blockDim.x / parts, bps = m / cpw;
    const uint32_t set = blockIdx.x / bps, part = tid / cpw, c = (blockIdx.x % bps) * cpw + tid % cpw;
    const uint32_t base = miss_start[set], count = miss_start[set + 1] - base;
    const uint32_t len = coset_recover_slice_len(count, parts), mine = coset_recover_slice_valid(count, parts, part);
    const Fr xd = vld_fr(roots + ((__brev(c) >> (19 + e)) << e)), xc = mul(vld_fr(shift + (1u << e)), xd);
    Fr pd = Fr::one(), pc = Fr::one();
    for (uint32_t t0 = 0; t0 < len; t0 += cpw) {
        {   // lane (q, tt) fetches step t0 + tt of part q; a step past the list reads roots[0] and is never used
            const uint32_t step = t0 + tid % cpw, i = part * len + step;
            const bool on = step < len && i < count;
            lds_st(sh_r, tid, vld_fr(roots + (on ? miss[base + i] : 0u)));
        }
        __syncthreads();
        const uint32_t steps = len - t0 < cpw ? len - t0 : cpw;
        const uint32_t valid = mine > t0 ? (mine - t0 < steps ? mine - t0 : steps) : 0u;
        coset_recover_chain(pd, pc, xd, xc, steps, valid, [&](uint32_t t) { return lds_ld(sh_r, part * cpw + t); });
        __syncthreads();
    }
    if (parts > 1) {
        lds_st(sh_d, tid, pd);
        lds_st(sh_c, tid, pc);
        for (uint32_t s2 = parts >> 1; s2 >= 1; s2 >>= 1) {
            __syncthreads();
            if (part < s2) {   // reads [s2 cpw, 2 s2 cpw), writes [0, s2 cpw)
                pd = mul(pd, lds_ld(sh_d, tid + s2 * cpw));
                pc = mul(pc, lds_ld(sh_c, tid + s2 * cpw));
                lds_st(sh_d, tid, pd);
                lds_st(sh_c, tid, pc);
            }
        }
    }
    if (part == 0) {
        vst_fr(z_domain + (size_t)set * m + c, pd);
        vst_fr(z_coset_inv + (size_t)set * m + c, fr_inv_dev(pc));
    }
}

// item i of the chunk's input (l values, 2 l uint4) -> image[coset_dst[i]], coset_dst = device row * m + coset; the image
// is zero elsewhere.  16 bytes per lane: two lanes per item at e = 0.
__global__ void k_scatter_cosets_rows(uint4 *image, const uint4 *in, const uint32_t *coset_dst, size_t total_u4, int e) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= total_u4) return;
    const uint32_t sub = (uint32_t)g & ((2u << e) - 1u);
    image[((size_t)coset_dst[g >> (e + 1)] << (e + 1)) + sub] = in[g];
}

// a[g] *= f[row_set[g >> 13]][(g & 8191) >> e]
__global__ void k_fr_mul_coset_factor(Fr *a, const Fr *f, const uint32_t *row_set, size_t n, int e) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint32_t set = row_set[g >> 13], coset = ((uint32_t)g & (COSET_RECOVER_EXT - 1u)) >> e;
    vst_fr(a + g, mul(vld_fr(a + g), vld_fr(f + (((size_t)set * COSET_RECOVER_EXT) >> e) + coset)));
}

int coset_recover_factors_enqueue(DeviceCtx *ctx, Fr *d_z_domain, Fr *d_z_coset_inv, const uint32_t *d_miss,
                                  const uint32_t *d_miss_start, size_t nsets, int e, uint32_t parts) {
    if (!nsets) return 0;
    if (e < 0 || e > COSET_RECOVER_MAX_LOG || parts == 0 || (parts & (parts - 1)) || parts > T / 4) return 2;
    const uint32_t block = coset_recover_block(e, parts), bps = coset_recover_cosets(e) / (block / parts);
    hipLaunchKernelGGL(k_coset_recover_factors, dim3((unsigned)(nsets * bps)), dim3(block), 0, ctx->stream, d_z_domain,
                       d_z_coset_inv, d_miss, d_miss_start, ctx->d_roots, ctx->d_shift, e, parts);
    HIP_TRY(hipGetLastError());
    return 0;
}

int scatter_cosets_rows_enqueue(DeviceCtx *ctx, uint8_t *d_image, const uint8_t *d_in, const uint32_t *d_coset_dst,
                                size_t ncosets, int e) {
    const size_t u4 = ncosets << (e + 1);
    if (!u4) return 0;
    hipLaunchKernelGGL(k_scatter_cosets_rows, dim3((unsigned)((u4 + 255) / 256)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<uint4 *>(d_image), reinterpret_cast<const uint4 *>(d_in), d_coset_dst, u4, e);
    HIP_TRY(hipGetLastError());
    return 0;
}

int fr_mul_coset_factor_enqueue(DeviceCtx *ctx, Fr *d_a, const Fr *d_f, const uint32_t *d_row_set, size_t nrows, int e) {
    const size_t n = nrows * COSET_RECOVER_EXT;
    if (!n) return 0;
    hipLaunchKernelGGL(k_fr_mul_coset_factor, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_a, d_f,
                       d_row_set, n, e);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace dev
}  // namespace ckzg
