// locate.hip -- the device half of the per-item verdicts at batch cost (ckzg_hip_verify_kzg_proof_batch_locate,
// ckzg_hip_verify_blob_kzg_proof_batch_locate; host glue: ckzg_api2.hip, locate_chunk_from_lhs):
//   * k_locate_scale: per item A_i = [r^i] P1_i and B_i = [r^i] proof_i, the terms of the batch check's two sums
//   * k_g1_scan_tiles / k_g1_scan_offsets: inclusive prefix sums over G1 points (XYZZ, complete addition), which is also
//     what ckzg_hip_g1_prefix_sums exposes on its own.
// With the prefix sums PA, PB on the host, any contiguous range [a, b) of the batch is checked there with two point
// subtractions and one two-pairing check; nothing more is asked of the device.
#include "device.hpp"
#include "g1_glv_dev.hpp"
#include "rpow2.hpp"

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
