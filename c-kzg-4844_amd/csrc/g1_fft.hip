// g1_fft.hip -- the G1 Fourier transform at any power of two up to 8192 (g1_fft / g1_ifft_unscaled,
// src/eip7594/fft.c:164-240) and, on top of it, one FK20 pipeline for the openings of a blob on every coset of 1 to 64
// points of the extended domain and at every point of the evaluation domain (src/eip7594/fk20.c at those cell sizes,
// setup.c:238-330 for the transformed setup).
//
// fk20.hip's transforms are hard-wired to length 128 and order their lanes transform-fastest, so that a wave holds ONE
// twiddle and the digit-driven NAF ladder stays uniform.  One transform of length 8192 has no such order: in the stages
// with fewer than 64 twiddle groups a wave holds 64 different twiddles.  So the ladders here have FIXED addition
// positions (4-bit windows, a per-lane table entry; xyzz28_mul_w4_128 and its four-lane form) and the lane order is free.
//
// A stage (butterfly span 2^s) is three launches on data in HBM, in place:
//   k_gfft_addsub    (u, v) <- (u + v, u - v) on every butterfly
//   k_gfft_ladder    the two GLV half-products [k1]P, [k2]phi(P) of every butterfly whose twiddle is not 1, each half
//                      on its own lane (or quad), into a scratch array: half the dependent chain of one lane doing both
//   k_gfft_sum       P <- the sum of its two half-products
// DIF (natural in, bit-reversed out) runs s = logn .. 1 as addsub, ladder, sum; DIT (bit-reversed in, natural out) runs
// s = 1 .. logn as ladder, sum, addsub.  Index maps: g1_fft_plan.hpp.
#include "device.hpp"
#include "dev_inline.hpp"
#include "g1_28.hpp"
#include "g1_quad.hpp"
#include "g1_fft_plan.hpp"

namespace ckzg {
namespace dev {

namespace {

__device__ __forceinline__ Fr ld_fr(const Fr *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    uint4 a = q[0], b = q[1];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}

// one GLV half-product on one lane (QUAD = false) or on the four lanes of a quad, which all pass the same arguments
template <bool QUAD>
__device__ __forceinline__ G1XYZZ half_product(XYZZ28 p, bool p_inf, const uint32_t *k128, bool second, int ql) {
    if (second) p.x = widen<1, 10>(mul(p.x, f28_const<1, 1>(FP28_BETA_LAMBDA)));   // phi(P) = (beta x, y)
    uint32_t k[4];
#pragma unroll
    for (int i = 0; i < 4; i++) k[i] = k128[i];
    XYZZ28 o;
    bool oi = true;
    if constexpr (QUAD)
        quad::xyzz28_mul_w4_128_quad(o, oi, p, p_inf, k, ql);
    else
        xyzz28_mul_w4_128(o, oi, p, p_inf, k);
    return xyzz28_to_xyzz(o, oi);
}

// the half-product this lane works on: `item` of `total`, the quad position; lanes (quads) past the end repeat the last
// item and store nothing, so that no wave runs the ladder partly masked
template <bool QUAD>
__device__ __forceinline__ bool ladder_item(size_t total, size_t &item, int &ql) {
    const size_t g = blockIdx.x * (size_t)64 + threadIdx.x;
    ql = QUAD ? (int)(threadIdx.x & 3) : 0;
    item = QUAD ? g >> 2 : g;
    const bool live = item < total;
    if (!live) item = total - 1;
    return live && ql == 0;
}

}  // namespace

// glv[i] = {k1[4], k2[4]} of w^i, i < 8192 (g1_28.hpp: glv_split; w = roots_of_unity[1])
__global__ __launch_bounds__(64) void k_gfft_roots(uint32_t *glv, const Fr *roots) {
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= (uint32_t)N_EXT) return;
    uint32_t raw[8];
    to_raw<FrParams>(raw, ld_fr(roots + g));
    glv_split(raw, glv + (size_t)g * 8, glv + (size_t)g * 8 + 4);
}

// tmp[(f * ladders + m) * 2 + h] = half-product h of slot i1(m) of transform f with the twiddle of butterfly m
template <bool QUAD>
__global__ __launch_bounds__(64) void k_gfft_ladder(
    G1XYZZ *tmp, const G1XYZZ *data, const uint32_t *roots_glv, uint32_t stride, uint32_t ladders, size_t total, int s,
    int inverse) {
    size_t item;
    int ql;
    const bool store = ladder_item<QUAD>(total, item, ql);
    const size_t bf = item >> 1;
    const bool second = (item & 1) != 0;
    const size_t f = bf / ladders;
    uint32_t i1, root;
    g1_fft_ladder_index((uint32_t)(bf - f * ladders), s, i1, root);
    if (inverse) root = (uint32_t)N_EXT - root;
    bool pi;
    const XYZZ28 p = xyzz28_from_xyzz(data[f * stride + i1], pi);
    const G1XYZZ r = half_product<QUAD>(p, pi, roots_glv + (size_t)root * 8 + (second ? 4 : 0), second, ql);
    if (store) tmp[item] = r;
}

// slot i1(m) of transform f <- tmp[2 (f * ladders + m)] + tmp[2 (f * ladders + m) + 1]
__global__ __launch_bounds__(64) void k_gfft_sum(G1XYZZ *data, const G1XYZZ *tmp, uint32_t stride, uint32_t ladders,
                                                   size_t total, int s) {
    const size_t bf = blockIdx.x * (size_t)64 + threadIdx.x;
    if (bf >= total) return;
    const size_t f = bf / ladders;
    uint32_t i1, root;
    g1_fft_ladder_index((uint32_t)(bf - f * ladders), s, i1, root);
    bool ai, bi;
    XYZZ28 a = xyzz28_from_xyzz(tmp[2 * bf], ai), b = xyzz28_from_xyzz(tmp[2 * bf + 1], bi);
    xyzz28_add(a, ai, b, bi);
    data[f * stride + i1] = xyzz28_to_xyzz(a, ai);
}

// (u, v) <- (u + v, u - v) on butterfly bf of transform f; half_n = n / 2 butterflies per transform
__global__ __launch_bounds__(64) void k_gfft_addsub(G1XYZZ *data, uint32_t stride, uint32_t half_n, size_t total, int s) {
    const size_t g = blockIdx.x * (size_t)64 + threadIdx.x;
    if (g >= total) return;
    const size_t f = g / half_n;
    const uint32_t bf = (uint32_t)(g - f * half_n), half = 1u << (s - 1), j = bf & (half - 1u);
    const uint32_t i0 = ((bf >> (s - 1)) << s) + j, i1 = i0 + half;
    G1XYZZ *vec = data + f * stride;
    bool ui, vi;
    XYZZ28 u = xyzz28_from_xyzz(vec[i0], ui), v = xyzz28_from_xyzz(vec[i1], vi);
    XYZZ28 x = u;
    bool xi = ui;
    xyzz28_add(x, xi, v, vi);
    vec[i0] = xyzz28_to_xyzz(x, xi);
    xyzz28_add(u, ui, xyzz28_neg(v), vi);
    vec[i1] = xyzz28_to_xyzz(u, ui);
}

uint64_t g1_fft_quad_max() {
    static const uint64_t v = (uint64_t)ab_knob("CKZG_HIP_G1_FFT_QUAD_MAX", (long)G1_FFT_QUAD_MAX_DEFAULT);
    return v;
}

int g1_fft_roots_ensure(DeviceCtx *ctx) {
    if (ctx->d_g1_fft_roots) return 0;
    DevTmp t;
    HIP_TRY(hipMalloc(&t.p, (size_t)N_EXT * 8 * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_gfft_roots, dim3(N_EXT / 64), dim3(64), 0, ctx->stream, static_cast<uint32_t *>(t.p), ctx->d_roots);
    HIP_TRY(hipGetLastError());
    ctx->d_g1_fft_roots = static_cast<uint32_t *>(t.p);   // (read by later launches on the same stream only)
    t.p = nullptr;
    return 0;
}

size_t g1_fft_tmp_points(int logn, size_t count) { return logn < 2 ? 0 : 2 * count * (size_t)g1_fft_ladders(logn, logn); }

// the launch of `products` half-product pairs in the form the picker names
template <class Launch>
static void launch_ladders(size_t products, Launch &&launch) {
    const bool quad = g1_fft_form(products, g1_fft_quad_max()) == G1_FFT_FORM_QUAD;
    const size_t lanes = 2 * products * (quad ? 4 : 1);
    launch(quad, dim3((unsigned)((lanes + 63) / 64)), 2 * products);
}

int g1_fft_enqueue(DeviceCtx *ctx, G1XYZZ *d_data, G1XYZZ *d_tmp, int logn, size_t count, size_t stride, bool dif, int inverse) {
    if (count == 0 || logn <= 0) return 0;
    if (logn > G1_FFT_MAX_LOG || stride < ((size_t)1 << logn) || count * stride > ((size_t)1 << 31)) return 2;
    int rc = g1_fft_roots_ensure(ctx);
    if (rc) return rc;
    const uint32_t half_n = 1u << (logn - 1);
    const size_t nbf = count * half_n;
    const dim3 block(64), bgrid((unsigned)((nbf + 63) / 64));
    for (int s = dif ? logn : 1; dif ? s >= 1 : s <= logn; s += dif ? -1 : 1) {
        if (dif) hipLaunchKernelGGL(k_gfft_addsub, bgrid, block, 0, ctx->stream, d_data, (uint32_t)stride, half_n, nbf, s);
        const uint32_t ladders = g1_fft_ladders(logn, s);
        if (ladders) {
            const size_t products = count * ladders;
            launch_ladders(products, [&](bool quad, dim3 grid, size_t total) {
                if (quad)
                    hipLaunchKernelGGL(k_gfft_ladder<true>, grid, block, 0, ctx->stream, d_tmp, d_data, ctx->d_g1_fft_roots,
                                       (uint32_t)stride, ladders, total, s, inverse);
                else
                    hipLaunchKernelGGL(k_gfft_ladder<false>, grid, block, 0, ctx->stream, d_tmp, d_data, ctx->d_g1_fft_roots,
                                       (uint32_t)stride, ladders, total, s, inverse);
            });
            hipLaunchKernelGGL(k_gfft_sum, dim3((unsigned)((products + 63) / 64)), block, 0, ctx->stream, d_data, d_tmp,
                               (uint32_t)stride, ladders, products, s);
        }
        if (!dif) hipLaunchKernelGGL(k_gfft_addsub, bgrid, block, 0, ctx->stream, d_data, (uint32_t)stride, half_n, nbf, s);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// FK20 openings on every coset of size l = 2^e, e <= 6 (src/eip7594/fk20.c at any cell size up to 64; setup.c:238-330
// for the transformed setup).  k = 4096 / l; the l Toeplitz columns of length 2k fill one row of 8192 column-major, for
// the scalars, the transformed setup and the products alike, so the scalar transform, the ladders and the sum of the
// GLV halves have one shape whatever e is.  Then the columns are added and the row's first 2k entries go through the
// inverse transform, whose first k entries are h, the Toeplitz product of the coefficients with the setup.  Nothing is
// permuted: the scalar transform and the setup transform are both DIF (bit-reversed out), their pointwise product
// feeds the DIT inverse (natural out), and h feeds a DIF forward transform.  Which one is the caller's choice:
//   of (h, 0) at length 2k: position c of the output is the proof of coset c of the bit-reversed extended domain;
//   at e = 0 also of h alone at length 4096: pi(w^brp12(j)), the proof of blob element j.  These are the first 4096
//   outputs of the length-8192 transform -- its first DIF stage leaves h in the lower half -- at half its cost.
// ------------------------------------------------------------------------------------------

// xin[t] = g1_values_monomial[coset_setup_source(t)], the identity where that is -1 (g1_fft_plan.hpp)
__global__ void k_coset_xext_gather(G1XYZZ *xin, const G1Affine *monomial, int e) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint32_t)N_EXT) return;
    const int src = coset_setup_source(t, e, (uint32_t)N_BLOB);
    xin[t] = src >= 0 ? xyzz_from_affine(monomial[src]) : G1XYZZ::inf();
}

// v[b][t]: the l circulant columns of blob b from its monomial coefficients (g1_fft_plan.hpp: coset_circulant_source)
__global__ void k_coset_circulant(Fr *v, const Fr *poly, size_t total, int e) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= total) return;
    const size_t b = g >> 13;
    const int src = coset_circulant_source((uint32_t)g & (uint32_t)(N_EXT - 1), e, (uint32_t)N_BLOB);
    const uint4 *q = reinterpret_cast<const uint4 *>(poly + b * N_BLOB + (src < 0 ? 0 : src));
    uint4 lo = q[0], hi = q[1];
    if (src < 0) lo = hi = make_uint4(0, 0, 0, 0);
    uint4 *o = reinterpret_cast<uint4 *>(v + g);
    o[0] = lo;
    o[1] = hi;
}

// glv[g] = the GLV halves of the canonical value of vhat[g] (Montgomery)
__global__ __launch_bounds__(64) void k_openings_scalars(uint32_t *glv, const Fr *vhat, size_t total) {
    const size_t g = blockIdx.x * (size_t)64 + threadIdx.x;
    if (g >= total) return;
    uint32_t raw[8];
    to_raw<FrParams>(raw, ld_fr(vhat + g));
    glv_split(raw, glv + g * 8, glv + g * 8 + 4);
}

// tmp[2 g + h] = half-product h of xhat[g mod 8192] with the scalar glv[g]
template <bool QUAD>
__global__ __launch_bounds__(64) void k_openings_ladder(
    G1XYZZ *tmp, const G1Affine *xhat, const uint32_t *glv, size_t total) {
    size_t item;
    int ql;
    const bool store = ladder_item<QUAD>(total, item, ql);
    const size_t g = item >> 1;
    const bool second = (item & 1) != 0;
    const G1Affine a = xhat[g & (size_t)(N_EXT - 1)];
    XYZZ28 p;
    p.x = widen<1, 10>(f28_from_fp(a.x));
    p.y = widen<1, 6>(f28_from_fp(a.y));
    p.zz = widen<1, 2>(f28_one());
    p.zzz = p.zz;
    const G1XYZZ r = half_product<QUAD>(p, a.is_inf(), glv + g * 8 + (second ? 4 : 0), second, ql);
    if (store) tmp[item] = r;
}

// u[g] = tmp[2 g] + tmp[2 g + 1]
__global__ __launch_bounds__(64) void k_openings_sum(G1XYZZ *u, const G1XYZZ *tmp, size_t total) {
    const size_t g = blockIdx.x * (size_t)64 + threadIdx.x;
    if (g >= total) return;
    bool ai, bi;
    XYZZ28 a = xyzz28_from_xyzz(tmp[2 * g], ai), b = xyzz28_from_xyzz(tmp[2 * g + 1], bi);
    xyzz28_add(a, ai, b, bi);
    u[g] = xyzz28_to_xyzz(a, ai);
}

// out48[g] = compress(aff[g])
__global__ void k_openings_compress(uint8_t *out48, const G1Affine *aff, size_t total) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= total) return;
    uint8_t buf[48];
    g1_compress_affine(buf, aff[g]);
    for (int k = 0; k < 48; k++) out48[g * 48 + k] = buf[k];
}

// Column sum, one strided pass: a row of 8192 points holds columns of 2^logw points; column `part` of row b <- the sum
// of its columns part, part + parts, ..., part + (ncols - 1) parts, at every position t.  One lane per (b, part, t), t
// fastest: a wave reads 64 consecutive points of one column per step.  In place: a lane reads and writes position t of
// the columns = part (mod parts) of its row, which no other lane of the launch touches.  The addition is complete.
__global__ __launch_bounds__(64) void k_coset_colsum(G1XYZZ *u, int logw, uint32_t parts, uint32_t ncols, size_t total) {
    const size_t g = blockIdx.x * (size_t)64 + threadIdx.x;
    if (g >= total) return;
    const size_t t = g & (((size_t)1 << logw) - 1), rest = g >> logw;
    const size_t b = rest / parts, part = rest - b * parts;
    G1XYZZ *col = u + b * N_EXT + (part << logw) + t;
    const size_t step = (size_t)parts << logw;
    bool ai;
    XYZZ28 a = xyzz28_from_xyzz(col[0], ai);
    for (uint32_t j = 1; j < ncols; j++) {
        bool pi;
        const XYZZ28 p = xyzz28_from_xyzz(col[j * step], pi);
        xyzz28_add(a, ai, p, pi);
    }
    col[0] = xyzz28_to_xyzz(a, ai);
}

// u[b][2^(logn-1) .. 2^logn - 1] <- the identity, on rows of 8192; total = rows * 2^(logn-1)
__global__ void k_coset_zero_upper(G1XYZZ *u, int logn, size_t total) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= total) return;
    const size_t half = (size_t)1 << (logn - 1);
    u[(g >> (logn - 1)) * N_EXT + half + (g & (half - 1))] = G1XYZZ::inf();
}

// u[b][t] <- sum_{i < 2^e} u[b][i * 2k + t] for t < 2k = 8192 >> e, on rows of 8192: one pass up to COSET_COLSUM_RADIX
// columns, two above (g1_fft_plan.hpp: coset_colsum_parts).  Enqueue-only.
int coset_colsum_enqueue(DeviceCtx *ctx, G1XYZZ *d_u, int e, size_t rows) {
    if (e < 0 || e > COSET_MAX_LOG || rows > ((size_t)1 << 17)) return 2;
    if (e == 0 || rows == 0) return 0;
    const int logw = G1_FFT_MAX_LOG - e;
    const uint32_t l = 1u << e, parts = coset_colsum_parts(e);
    if (parts > 1) {
        const size_t total = (rows * parts) << logw;
        hipLaunchKernelGGL(k_coset_colsum, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, ctx->stream, d_u, logw, parts, l / parts, total);
    }
    const size_t total = rows << logw;
    hipLaunchKernelGGL(k_coset_colsum, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, ctx->stream, d_u, logw, 1u,
                       parts > 1 ? parts : l, total);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The transformed setup of coset size 2^e, this slot's own: the l columns, each through the forward transform of length
// 2k, affine, DIF order.  Built by the slot's first call with that e, kept until the slot goes; a failure keeps
// nothing.
int openings_xhat_ensure(DeviceCtx *ctx, int e) {
    if (e < 0 || e > COSET_MAX_LOG) return 2;
    if (ctx->d_openings_xhat[e]) return 0;
    int rc = g1_fft_roots_ensure(ctx);
    if (rc) return rc;
    const int logn = G1_FFT_MAX_LOG - e;
    const size_t l = (size_t)1 << e;
    DevTmp xin, tmp, prefix, out;   // gone on every exit path
    HIP_TRY(hipMalloc(&xin.p, (size_t)N_EXT * sizeof(G1XYZZ)));
    HIP_TRY(hipMalloc(&tmp.p, g1_fft_tmp_points(logn, l) * sizeof(G1XYZZ)));
    HIP_TRY(hipMalloc(&prefix.p, (size_t)N_EXT * sizeof(Fp)));
    HIP_TRY(hipMalloc(&out.p, (size_t)N_EXT * sizeof(G1Affine)));
    // (the three temporaries; `out` is the table that stays)
    HIP_TRY(poison_fresh(xin.p, (size_t)N_EXT * sizeof(G1XYZZ), ctx->stream));
    HIP_TRY(poison_fresh(tmp.p, g1_fft_tmp_points(logn, l) * sizeof(G1XYZZ), ctx->stream));
    HIP_TRY(poison_fresh(prefix.p, (size_t)N_EXT * sizeof(Fp), ctx->stream));
    G1XYZZ *d_xin = static_cast<G1XYZZ *>(xin.p);
    hipLaunchKernelGGL(k_coset_xext_gather, dim3(N_EXT / 256), dim3(256), 0, ctx->stream, d_xin, ctx->d_mono, e);
    rc = g1_fft_enqueue(ctx, d_xin, static_cast<G1XYZZ *>(tmp.p), logn, l, (size_t)1 << logn, /*dif=*/true, /*inverse=*/0);
    if (!rc) rc = batch_to_affine_device(ctx, static_cast<G1Affine *>(out.p), d_xin, static_cast<Fp *>(prefix.p), N_EXT);
    // the scratch is freed when this function returns: nothing may still be running on it, error or not
    if (dev::sync_stream(ctx->stream) != hipSuccess && !rc) rc = 2;
    if (rc) return rc;
    ctx->d_openings_xhat[e] = static_cast<G1Affine *>(out.p);
    out.p = nullptr;
    return 0;
}

static size_t al256(size_t v) { return (v + 255) / 256 * 256; }

// the coefficients, the scalars and their GLV halves, the rows u and the ladders' halves; the affine points and the
// inversion prefixes of the output (up to 8192 per blob) lie on the rows of u once these have been gathered
size_t openings_scratch_bytes(size_t k) {
    return al256(k * N_BLOB * sizeof(Fr)) + al256(k * N_EXT * sizeof(Fr)) + al256(k * N_EXT * 8 * sizeof(uint32_t)) +
           al256(k * N_EXT * sizeof(G1XYZZ)) + al256(2 * k * N_EXT * sizeof(G1XYZZ));
}

// d_blobs[k] (bytes) -> d_proofs48[k][2^out_log] and, if d_evals != nullptr, d_evals[k][8192][32], the extended
// evaluations in cell order; d_bad[k] (zeroed by the caller on the stream) |= 1 for a blob with a non-canonical element.
// out_log is the log length of the last forward transform: 13 - e, on (h, 0), for the proofs of every coset; at e = 0
// also 12, on h alone, for those of the evaluation domain.  Enqueue-only, on ctx->stream; `scratch` holds
// openings_scratch_bytes(k).
int openings_enqueue(DeviceCtx *ctx, uint8_t *d_proofs48, uint8_t *d_evals, uint32_t *d_bad, const uint8_t *d_blobs, size_t k,
                     int e, int out_log, uint8_t *scratch) {
    if (k == 0) return 0;
    if (e < 0 || e > COSET_MAX_LOG || k > ((size_t)1 << 17)) return 2;
    const int logn = G1_FFT_MAX_LOG - e;
    if (out_log != logn && !(e == 0 && out_log == logn - 1)) return 2;
    const G1Affine *xhat = ctx->d_openings_xhat[e];
    if (!xhat) return 2;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t *p = scratch + off;
        off += al256(bytes);
        return p;
    };
    Fr *poly = reinterpret_cast<Fr *>(take(k * N_BLOB * sizeof(Fr)));
    Fr *v = reinterpret_cast<Fr *>(take(k * N_EXT * sizeof(Fr)));
    uint32_t *glv = reinterpret_cast<uint32_t *>(take(k * N_EXT * 8 * sizeof(uint32_t)));
    G1XYZZ *u = reinterpret_cast<G1XYZZ *>(take(k * N_EXT * sizeof(G1XYZZ)));
    G1XYZZ *tmp = reinterpret_cast<G1XYZZ *>(take(2 * k * N_EXT * sizeof(G1XYZZ)));
    const size_t m = (size_t)1 << out_log, nout = k * m;
    // the output's affine points and prefixes: on u, once its rows have been gathered into tmp
    G1Affine *aff = reinterpret_cast<G1Affine *>(u);
    Fp *prefix = reinterpret_cast<Fp *>(reinterpret_cast<uint8_t *>(u) + al256(nout * sizeof(G1Affine)));
    static_assert(sizeof(G1Affine) + sizeof(Fp) + 1 <= sizeof(G1XYZZ), "the output's affine form fits the rows of u");
    // monomial coefficients and, if wanted, the extended evaluations (v is their scratch); the l circulant columns,
    // each through its transform / 2k
    int rc = cells_stage_enqueue(ctx, d_evals, poly, v, d_bad, d_blobs, k);
    if (rc) return rc;
    const size_t total = k * N_EXT;
    hipLaunchKernelGGL(k_coset_circulant, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, v, poly, total, e);
    HIP_TRY(hipGetLastError());
    rc = fr_ntt_batch(ctx, v, k << e, logn, /*dif=*/true, /*inverse=*/false, /*scale=*/true);
    if (rc) return rc;
    // product[i][t] = vhat_i[t] xhat_i[t], both in the DIF output order; u[t] = their sum over the columns
    hipLaunchKernelGGL(k_openings_scalars, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, ctx->stream, glv, v, total);
    launch_ladders(total, [&](bool quad, dim3 grid, size_t items) {
        if (quad)
            hipLaunchKernelGGL(k_openings_ladder<true>, grid, dim3(64), 0, ctx->stream, tmp, xhat, glv, items);
        else
            hipLaunchKernelGGL(k_openings_ladder<false>, grid, dim3(64), 0, ctx->stream, tmp, xhat, glv, items);
    });
    hipLaunchKernelGGL(k_openings_sum, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, ctx->stream, u, tmp, total);
    HIP_TRY(hipGetLastError());
    rc = coset_colsum_enqueue(ctx, u, e, k);
    if (rc) return rc;
    // h = the first half of the unscaled inverse transform of length 2^logn; proofs = the forward transform of (h, 0) at
    // that length, or of h alone at half of it, which never reads the upper half; in place in the heads of the rows
    rc = g1_fft_enqueue(ctx, u, tmp, logn, k, N_EXT, /*dif=*/false, /*inverse=*/1);
    if (rc) return rc;
    if (out_log == logn)
        hipLaunchKernelGGL(k_coset_zero_upper, dim3((unsigned)((nout / 2 + 255) / 256)), dim3(256), 0, ctx->stream, u, logn, nout / 2);
    rc = g1_fft_enqueue(ctx, u, tmp, out_log, k, N_EXT, /*dif=*/true, /*inverse=*/0);
    if (rc) return rc;
    // the heads of the rows, contiguous (tmp is free again), normalised and compressed
    HIP_TRY(hipMemcpy2DAsync(tmp, m * sizeof(G1XYZZ), u, (size_t)N_EXT * sizeof(G1XYZZ), m * sizeof(G1XYZZ), k,
                             hipMemcpyDeviceToDevice, ctx->stream));
    rc = batch_to_affine_device(ctx, aff, tmp, prefix, nout);
    if (rc) return rc;
    hipLaunchKernelGGL(k_openings_compress, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, ctx->stream, d_proofs48, aff, nout);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace dev
}  // namespace ckzg
