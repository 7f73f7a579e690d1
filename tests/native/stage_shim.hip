// stage_shim.hip -- the stages that turn a batch challenge into scalars, and the items into the bytes that are hashed,
// behind a C ABI (tests/test_gpu_rlc_stages.py): rlc_scalars_enqueue, coset_rlc_scalars_enqueue at
// cosets of 64 (the scalars of a cell batch), coset_group_rlc_scalars_enqueue at cosets of 64, blob_group_scalars_enqueue, locate_scale_enqueue, batch_transcript_rows_device and
// rpow2.hpp's rpow_at.  A weight of a batch check is the one value no verdict can check -- any consistent weights pass an
// honest batch and fail a spoilt one -- so these values are read here and compared with integers.
//
// This file is linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libstage_shim.so), so every kernel but ss_k_rpow_at
// is the product's binary code, not a second compilation.  The stage functions need `stream` and `d_roots` of their
// DeviceCtx and nothing else: no trusted setup, no tables.  Test aid only; its exports are ss_* and none of them is
// part of libckzg_hip.so.
//
// Calling convention (dev_shim_common.hpp): host pointers in and out, a stream of its own per call, a polling 20 s
// deadline, a non-zero return on any HIP error.  Scalars cross as canonical little-endian limbs (8 words), also
// where the product keeps them in Montgomery form (d_rp, d_ry); points as 144-byte Jacobian strings (X | Y | Z in
// Montgomery form, all zero = infinity), affine (Z = 1) where they go in.  Every output buffer comes back whole, padding
// included.
#include <cstring>
#include "dev_shim_common.hpp"
#include "device.hpp"
#include "rpow2.hpp"
#include "blob_groups_plan.hpp"
#include "coset_groups_plan.hpp"

using namespace ckzg;
using namespace ckzg::dev;

namespace {

constexpr int CELL_LOG = 6;   // a cell is a coset of 64 values
constexpr size_t SS_MAX_ITEMS = (size_t)1 << 20;   // no call of a test comes near; keeps every buffer small

std::vector<Fr> fr_in(const uint32_t *raw, size_t n) {
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; i++) v[i] = from_raw<FrParams>(raw + 8 * i);
    return v;
}
void fr_out(uint32_t *raw, const std::vector<Fr> &v) {
    for (size_t i = 0; i < v.size(); i++) to_raw<FrParams>(raw + 8 * i, v[i]);
}
// an affine point from a 144-byte string: Z must be 1 (Montgomery) or the whole string zero
bool affine_in(G1Affine &out, const uint8_t *p144) {
    G1Jac j;
    memcpy(&j, p144, sizeof(G1Jac));
    if (j.is_inf()) {
        out = G1Affine::inf();
        return true;
    }
    const Fp one = Fp::one();
    if (memcmp(&j.z, &one, sizeof(Fp)) != 0) return false;
    out = {j.x, j.y};
    return true;
}

// all a stage function reads of its context
void stage_ctx(DeviceCtx &ctx, hipStream_t st, Fr *d_roots) {
    ctx.stream = st;
    ctx.d_roots = d_roots;
}

}  // namespace

__global__ __launch_bounds__(64) void ss_k_rpow_at(uint32_t *out, const uint32_t *idx, RPow2 t, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t raw[8];
    to_raw<FrParams>(raw, rpow_at(t, idx[i]));
    for (int k = 0; k < 8; k++) out[(size_t)i * 8 + k] = raw[k];
}

extern "C" {

static_assert(sizeof(G1Jac) == 144 && sizeof(G1Affine) == 96 && sizeof(Fr) == 32, "the strings the tests pass");

// out[i] = r^idx[i], idx[i] < 2^24
int ss_rpow_at(uint32_t *out, const uint32_t *r, const uint32_t *idx, int n) {
    if (n <= 0 || (size_t)n > SS_MAX_ITEMS) return DS_BAD_ARG;
    for (int i = 0; i < n; i++)
        if (idx[i] >> 24) return DS_BAD_ARG;
    const RPow2 t = rpow2_of(from_raw<FrParams>(r));
    std::vector<Arg> args = {{nullptr, out, (size_t)n * 32}, {idx, nullptr, (size_t)n * 4}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(ss_k_rpow_at, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (uint32_t *)args[0].dev,
                           (const uint32_t *)args[1].dev, t, n);
    });
}

// sc [6 n][8]: goes up as the caller filled it (the stage clears it itself) and comes back whole
int ss_rlc_scalars(uint32_t *sc, const uint32_t *z, const uint32_t *r, size_t n) {
    if (!n || n > SS_MAX_ITEMS) return DS_BAD_ARG;
    const std::vector<Fr> zf = fr_in(z, n);
    const Fr rf = from_raw<FrParams>(r);
    std::vector<Arg> args = {{sc, sc, 6 * n * 32}, {zf.data(), nullptr, n * 32}};
    int rc = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        rc = rlc_scalars_enqueue(st, (uint32_t *)args[0].dev, (const Fr *)args[1].dev, rf, n);
    });
    return run ? run : rc;
}

// The scalars of a cell batch: coset_rlc_scalars_enqueue at cosets of 64 (the stage at every coset size, with guards
// around its buffers: coset_verify_shim.hip).  rp [n][8] (canonical), vec_rp [n][8], vec_wrp [n][8], vec_w [nc][8];
// cell_idx [n] < 128; roots: w^i, 8193 of them
int ss_cell_rlc_scalars(uint32_t *rp, uint32_t *vec_rp, uint32_t *vec_wrp, uint32_t *vec_w, const uint32_t *cell_idx,
                        const uint32_t *grp_start, const uint32_t *members, const uint32_t *r, const uint32_t *roots, size_t n,
                        size_t nc) {
    if (!n || n > SS_MAX_ITEMS || !nc || nc > n) return DS_BAD_ARG;
    if (grp_start[0] != 0 || grp_start[nc] != n) return DS_BAD_ARG;
    for (size_t j = 0; j < nc; j++)
        if (grp_start[j] > grp_start[j + 1]) return DS_BAD_ARG;
    for (size_t m = 0; m < n; m++)
        if (members[m] >= n || cell_idx[m] >= 128) return DS_BAD_ARG;
    const std::vector<Fr> rootsf = fr_in(roots, 8193);
    const Fr rf = from_raw<FrParams>(r);
    std::vector<Fr> rpf(n);
    std::vector<Arg> args = {{nullptr, rpf.data(), n * 32},        {nullptr, vec_rp, n * 32},
                             {nullptr, vec_wrp, n * 32},           {nullptr, vec_w, nc * 32},
                             {cell_idx, nullptr, n * 4},           {grp_start, nullptr, (nc + 1) * 4},
                             {members, nullptr, n * 4},            {rootsf.data(), nullptr, rootsf.size() * 32}};
    int rc = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        stage_ctx(ctx, st, (Fr *)args[7].dev);
        rc = coset_rlc_scalars_enqueue(&ctx, (Fr *)args[0].dev, (uint32_t *)args[1].dev, (uint32_t *)args[2].dev,
                                       (uint32_t *)args[3].dev, (const uint32_t *)args[4].dev, (const uint32_t *)args[5].dev,
                                       (const uint32_t *)args[6].dev, rf, n, nc, CELL_LOG);
    });
    if (run || rc) return run ? run : rc;
    fr_out(rp, rpf);
    return 0;
}

// The scalars of a chunk of cell groups: coset_group_rlc_scalars_enqueue at cosets of 64 (the stage at every coset size,
// with guards around its buffers: coset_groups_shim.hip).  The index maps are the product's (build_coset_groups_plan at
// e = 6).  Out, as hs_cell_groups_replay gives them: info = total,
// quad, pairs, rows; term_src [total]; part_off [2 G + 1]; sc [total][8] -- here with the terms of the interpolation
// commitment left as the caller of the stage zeroed them -- and rp [N][8] (canonical).  r: the groups' challenges.
// DS_BAD_ARG if the layout exceeds cap_terms.
int ss_cell_groups_scalars(uint32_t *sc, uint32_t *rp, uint32_t *term_src, uint32_t *part_off, uint32_t *info, size_t cap_terms,
                           const uint64_t *start, size_t G, const uint32_t *cell_commit, size_t num_commits,
                           const uint64_t *cell_indices, const uint32_t *r, const uint32_t *roots, size_t quad_max_terms) {
    if (!G || start[0] != 0) return DS_BAD_ARG;
    for (size_t g = 0; g < G; g++)
        if (start[g] > start[g + 1]) return DS_BAD_ARG;
    const size_t N = (size_t)start[G];
    if (!N || N > SS_MAX_ITEMS) return DS_BAD_ARG;
    for (size_t i = 0; i < N; i++)
        if (cell_commit[i] >= num_commits) return DS_BAD_ARG;
    CosetGroupsPlan p;
    build_coset_groups_plan(p, start, G, cell_commit, num_commits, cell_indices, CELL_LOG, quad_max_terms);
    if (p.total > cap_terms) return DS_BAD_ARG;
    info[0] = (uint32_t)p.total;
    info[1] = p.quad ? 1 : 0;
    info[2] = (uint32_t)p.P;
    info[3] = (uint32_t)p.R;
    for (size_t t = 0; t < p.total; t++) term_src[t] = p.term_src[t];
    for (size_t j = 0; j <= 2 * G; j++) part_off[j] = p.part_off[j];
    const std::vector<Fr> rootsf = fr_in(roots, 8193), rf = fr_in(r, G);
    std::vector<Fr> rpf(N);
    std::vector<Arg> args = {{nullptr, rpf.data(), N * 32},
                             {nullptr, sc, p.total * 32},
                             {p.item_grp.data(), nullptr, N * 4},
                             {p.item_col.data(), nullptr, N * 4},
                             {p.gd.data(), nullptr, p.gd.size() * 4},
                             {rf.data(), nullptr, G * 32},
                             {p.pair_start.data(), nullptr, p.pair_start.size() * 4},
                             {p.pair_members.data(), nullptr, p.pair_members.size() * 4},
                             {p.pair_term.data(), nullptr, p.pair_term.size() * 4},
                             {rootsf.data(), nullptr, rootsf.size() * 32}};
    int rc = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        stage_ctx(ctx, st, (Fr *)args[9].dev);
        rc = coset_group_rlc_scalars_enqueue(&ctx, (Fr *)args[0].dev, (uint32_t *)args[1].dev, (const uint32_t *)args[2].dev,
                                             (const uint32_t *)args[3].dev, (const uint32_t *)args[4].dev, (const Fr *)args[5].dev,
                                             (const uint32_t *)args[6].dev, (const uint32_t *)args[7].dev,
                                             (const uint32_t *)args[8].dev, N, G, p.P, CELL_LOG);
    });
    if (run || rc) return run ? run : rc;
    fr_out(rp, rpf);
    return 0;
}

// The index maps are the product's (build_blob_groups_plan).  Out, as hs_blob_groups_replay gives them: info = total,
// quad; term_src [total]; part_off [2 G + 1]; sc [total][8]; and ry [N][8] (canonical): r_g^(i - a) y_i.
int ss_blob_groups_scalars(uint32_t *sc, uint32_t *ry, uint32_t *term_src, uint32_t *part_off, uint32_t *info, size_t cap_terms,
                           const uint64_t *start, size_t G, const uint32_t *z, const uint32_t *y, const uint32_t *r,
                           size_t quad_max_terms) {
    if (!G || start[0] != 0) return DS_BAD_ARG;
    for (size_t g = 0; g < G; g++)
        if (start[g] > start[g + 1]) return DS_BAD_ARG;
    const size_t N = (size_t)start[G];
    if (!N || N > SS_MAX_ITEMS) return DS_BAD_ARG;
    BlobGroupsPlan p;
    build_blob_groups_plan(p, start, G, quad_max_terms);
    if (p.total > cap_terms) return DS_BAD_ARG;
    info[0] = (uint32_t)p.total;
    info[1] = p.quad ? 1 : 0;
    for (size_t t = 0; t < p.total; t++) term_src[t] = p.term_src[t];
    for (size_t j = 0; j <= 2 * G; j++) part_off[j] = p.part_off[j];
    const std::vector<Fr> zf = fr_in(z, N), yf = fr_in(y, N), rf = fr_in(r, G);
    std::vector<Fr> ryf(N);
    std::vector<Arg> args = {{nullptr, sc, p.total * 32},
                             {nullptr, ryf.data(), N * 32},
                             {p.blob_grp.data(), nullptr, N * 4},
                             {p.gd.data(), nullptr, p.gd.size() * 4},
                             {rf.data(), nullptr, G * 32},
                             {zf.data(), nullptr, N * 32},
                             {yf.data(), nullptr, N * 32}};
    int rc = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        stage_ctx(ctx, st, nullptr);
        rc = blob_group_scalars_enqueue(&ctx, (uint32_t *)args[0].dev, (Fr *)args[1].dev, (const uint32_t *)args[2].dev,
                                        (const uint32_t *)args[3].dev, (const Fr *)args[4].dev, (const Fr *)args[5].dev,
                                        (const Fr *)args[6].dev, N, G);
    });
    if (run || rc) return run ? run : rc;
    fr_out(ry, ryf);
    return 0;
}

// ab [2 n][144]: A_i = [r^i] p1[i], then B_i = [r^i] proof_i from neg_proof[i] = -proof_i; p1, neg_proof [n][144], affine
int ss_locate_scale(uint8_t *ab, const uint8_t *p1, const uint8_t *neg_proof, const uint32_t *r, size_t n) {
    if (!n || n > SS_MAX_ITEMS) return DS_BAD_ARG;
    std::vector<G1Affine> a(n), np(n);
    for (size_t i = 0; i < n; i++)
        if (!affine_in(a[i], p1 + 144 * i) || !affine_in(np[i], neg_proof + 144 * i)) return DS_BAD_ARG;
    const Fr rf = from_raw<FrParams>(r);
    std::vector<G1XYZZ> out(2 * n);
    std::vector<Arg> args = {{nullptr, out.data(), 2 * n * sizeof(G1XYZZ)},
                             {a.data(), nullptr, n * sizeof(G1Affine)},
                             {np.data(), nullptr, n * sizeof(G1Affine)}};
    int rc = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        stage_ctx(ctx, st, nullptr);
        rc = locate_scale_enqueue(&ctx, (G1XYZZ *)args[0].dev, (const G1Affine *)args[1].dev, (const G1Affine *)args[2].dev, rf, n);
    });
    if (run || rc) return run ? run : rc;
    for (size_t i = 0; i < 2 * n; i++) {
        const G1Jac j = out[i].is_inf() ? G1Jac::inf() : jac_from_xyzz(out[i]);
        memcpy(ab + 144 * i, &j, sizeof(G1Jac));
    }
    return 0;
}

// rows [n][160]; pts48: commitments [0, n), proofs [n, 2 n), 48 bytes each, as they are
int ss_batch_transcript_rows(uint8_t *rows, const uint8_t *pts48, const uint32_t *z, const uint32_t *y, size_t n) {
    if (!n || n > SS_MAX_ITEMS) return DS_BAD_ARG;
    const std::vector<Fr> zf = fr_in(z, n), yf = fr_in(y, n);
    std::vector<Arg> args = {{nullptr, rows, n * 160}, {pts48, nullptr, 2 * n * 48}, {zf.data(), nullptr, n * 32},
                             {yf.data(), nullptr, n * 32}};
    int rc = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        stage_ctx(ctx, st, nullptr);
        rc = batch_transcript_rows_device(&ctx, (uint8_t *)args[0].dev, (const uint8_t *)args[1].dev, (const Fr *)args[2].dev,
                                          (const Fr *)args[3].dev, n);
    });
    return run ? run : rc;
}

}  // extern "C"
