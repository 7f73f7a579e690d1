// coset_groups_shim.hip -- the device stages of ckzg_hip_verify_coset_kzg_proof_batch_groups (coset_groups.hip: the
// segmented scalars and weights, the aggregate over the chunk's rows, the rows' interpolation and the per-group sum)
// behind a C ABI (tests/test_gpu_coset_groups_stages.py), at every coset size 2^e.  The call itself reaches them with
// the challenges of its transcripts; here the challenges, the items and their cosets are the caller's.
//
// Linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libcoset_groups_shim.so), so the kernels are the product's binary
// code; the shim launches no kernel of its own.  The index maps are the product's too: every function builds the plan
// of coset_groups_plan.hpp from the chunk the caller describes (CgsChunk) and uploads its maps as the call does.  The
// stages need the stream and d_roots of their DeviceCtx and nothing else.  Test aid only; its exports are cgs_* and
// none of them is part of libckzg_hip.so.
//
// Calling convention (dev_shim_common.hpp): host pointers in and out, a stream of its own per call, a polling 20 s
// deadline, a non-zero return on any HIP error; what the stage itself returned goes to *rc.  Field elements cross as
// canonical little-endian limbs (8 words), also where the stage holds them in Montgomery form -- such a buffer is
// converted whole, guards included, so what a caller pre-fills it with must be < r.  Every buffer a stage writes goes
// up as the caller filled it with CGS_GUARD elements in front of the data and CGS_GUARD behind, and comes back whole.
#include <cstring>
#include "dev_shim_common.hpp"
#include "device.hpp"
#include "coset_groups_plan.hpp"

using namespace ckzg;
using namespace ckzg::dev;

extern "C" {
// a chunk: G groups over start[G] items; item_commit [N] < num_commits; coset_indices [N] < 8192 >> e
struct CgsChunk {
    const uint64_t *start;
    uint64_t G;
    const uint32_t *item_commit;
    uint64_t num_commits;
    const uint64_t *coset_indices;
    int32_t e;
    uint64_t quad_max_terms;
};
}

namespace {

constexpr size_t CGS_GUARD = 64;
constexpr size_t CGS_MAX_ITEMS = 1 << 14, CGS_MAX_GROUPS = 1 << 13, CGS_MAX_ELEMS = (size_t)1 << 20;

std::vector<Fr> fr_in(const uint32_t *raw, size_t n) {
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; i++) v[i] = from_raw<FrParams>(raw + 8 * i);
    return v;
}
void fr_out(uint32_t *raw, const std::vector<Fr> &v) {
    for (size_t i = 0; i < v.size(); i++) to_raw<FrParams>(raw + 8 * i, v[i]);
}

// the chunk is well formed and small enough: the plan
bool plan_of(CosetGroupsPlan &p, const CgsChunk *c) {
    if (!c || c->e < 0 || c->e > COSET_MAX_LOG || !c->G || c->G > CGS_MAX_GROUPS || !c->start || c->start[0] != 0) return false;
    for (size_t g = 0; g < c->G; g++)
        if (c->start[g] > c->start[g + 1]) return false;
    const size_t N = (size_t)c->start[c->G];
    if (!N || N > CGS_MAX_ITEMS || (N << c->e) > CGS_MAX_ELEMS || !c->num_commits || c->num_commits > N) return false;
    for (size_t i = 0; i < N; i++)
        if (c->item_commit[i] >= c->num_commits || c->coset_indices[i] >= coset_verify_cosets(c->e)) return false;
    build_coset_groups_plan(p, c->start, (size_t)c->G, c->item_commit, (size_t)c->num_commits, c->coset_indices, c->e,
                            (size_t)c->quad_max_terms);
    return true;
}

}  // namespace

extern "C" {

static_assert(sizeof(Fr) == 32, "the limbs the tests pass");

size_t cgs_guard() { return CGS_GUARD; }

// info [6] <- terms of the jobs (padded), quad, pairs, rows, parts of the aggregation, parts of the per-group sum
int cgs_plan_info(uint32_t *info, const CgsChunk *c) {
    CosetGroupsPlan p;
    if (!plan_of(p, c)) return DS_BAD_ARG;
    info[0] = (uint32_t)p.total;
    info[1] = p.quad ? 1 : 0;
    info[2] = (uint32_t)p.P;
    info[3] = (uint32_t)p.R;
    info[4] = coset_groups_agg_parts(p.N, p.R);
    info[5] = coset_groups_sum_parts(p.R, p.G);
    return 0;
}

// rp [GD + N + GD][8] (values < r) and sc [GD + total + GD][8] (canonical, as the stage writes them) go up as the
// caller filled them; r [G][8]; roots [8193][8]
int cgs_rlc_scalars(uint32_t *rp, uint32_t *sc, const CgsChunk *c, const uint32_t *r, const uint32_t *roots, int *rc) {
    CosetGroupsPlan p;
    if (!plan_of(p, c)) return DS_BAD_ARG;
    const size_t GD = CGS_GUARD, N = p.N, G = p.G;
    std::vector<Fr> rpv = fr_in(rp, N + 2 * GD);
    const std::vector<Fr> rootv = fr_in(roots, COSET_VERIFY_EXT + 1), rv = fr_in(r, G);
    std::vector<Arg> args = {{rpv.data(), rpv.data(), rpv.size() * 32, nullptr},
                             {sc, sc, (p.total + 2 * GD) * 32, nullptr},
                             {p.item_grp.data(), nullptr, N * 4, nullptr},
                             {p.item_col.data(), nullptr, N * 4, nullptr},
                             {p.gd.data(), nullptr, p.gd.size() * 4, nullptr},
                             {rv.data(), nullptr, G * 32, nullptr},
                             {p.pair_start.data(), nullptr, p.pair_start.size() * 4, nullptr},
                             {p.pair_members.data(), nullptr, N * 4, nullptr},
                             {p.pair_term.data(), nullptr, p.P * 4, nullptr},
                             {rootv.data(), nullptr, rootv.size() * 32, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        ctx.d_roots = (Fr *)args[9].dev;
        *rc = coset_group_rlc_scalars_enqueue(&ctx, (Fr *)args[0].dev + GD, (uint32_t *)args[1].dev + 8 * GD, (const uint32_t *)args[2].dev,
                                              (const uint32_t *)args[3].dev, (const uint32_t *)args[4].dev, (const Fr *)args[5].dev,
                                              (const uint32_t *)args[6].dev, (const uint32_t *)args[7].dev, (const uint32_t *)args[8].dev,
                                              N, G, p.P, p.e);
    });
    if (run) return run;
    fr_out(rp, rpv);
    return 0;
}

// rows [GD + R l + GD][8] goes up as the caller filled it (values < r); item_fr [N l][8]; rp [N][8]
int cgs_aggregate(uint32_t *rows, const uint32_t *item_fr, const uint32_t *rp, const CgsChunk *c, int *rc) {
    CosetGroupsPlan p;
    if (!plan_of(p, c)) return DS_BAD_ARG;
    const size_t GD = CGS_GUARD, N = p.N, slots = p.R << p.e;
    std::vector<Fr> out = fr_in(rows, slots + 2 * GD);
    const std::vector<Fr> iv = fr_in(item_fr, N << p.e), rv = fr_in(rp, N);
    std::vector<Arg> args = {{out.data(), out.data(), out.size() * 32, nullptr},
                             {iv.data(), nullptr, iv.size() * 32, nullptr},
                             {rv.data(), nullptr, N * 32, nullptr},
                             {p.row_start.data(), nullptr, p.row_start.size() * 4, nullptr},
                             {p.row_order.data(), nullptr, N * 4, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = coset_group_aggregate_device(&ctx, (Fr *)args[0].dev + GD, (const Fr *)args[1].dev, (const Fr *)args[2].dev,
                                           (const uint32_t *)args[3].dev, (const uint32_t *)args[4].dev, N, p.R, p.e);
    });
    if (run) return run;
    fr_out(rows, out);
    return 0;
}

// rows [GD + R l + GD][8] in (the aggregate) and out (each row's coefficients, coset factors taken out), values < r;
// roots [8193][8]
int cgs_interp(uint32_t *rows, const CgsChunk *c, const uint32_t *roots, int *rc) {
    CosetGroupsPlan p;
    if (!plan_of(p, c)) return DS_BAD_ARG;
    const size_t GD = CGS_GUARD, slots = p.R << p.e;
    std::vector<Fr> rowv = fr_in(rows, slots + 2 * GD);
    const std::vector<Fr> rootv = fr_in(roots, COSET_VERIFY_EXT + 1);
    std::vector<Arg> args = {{rowv.data(), rowv.data(), rowv.size() * 32, nullptr},
                             {p.row_col.data(), nullptr, p.R * 4, nullptr},
                             {rootv.data(), nullptr, rootv.size() * 32, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        ctx.d_roots = (Fr *)args[2].dev;
        *rc = coset_group_interp_device(&ctx, (Fr *)args[0].dev + GD, (const uint32_t *)args[1].dev, p.R, p.e);
    });
    if (run) return run;
    fr_out(rows, rowv);
    return 0;
}

// sc [GD + total + GD][8] goes up as the caller filled it (canonical); rows [R l][8]: what cgs_interp leaves
int cgs_interp_sum(uint32_t *sc, const uint32_t *rows, const CgsChunk *c, int *rc) {
    CosetGroupsPlan p;
    if (!plan_of(p, c)) return DS_BAD_ARG;
    const size_t GD = CGS_GUARD, slots = p.R << p.e;
    const std::vector<Fr> rowv = fr_in(rows, slots);
    std::vector<Arg> args = {{sc, sc, (p.total + 2 * GD) * 32, nullptr},
                             {rowv.data(), nullptr, slots * 32, nullptr},
                             {p.grp_rows.data(), nullptr, p.grp_rows.size() * 4, nullptr},
                             {p.gd.data(), nullptr, p.gd.size() * 4, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = coset_group_interp_sum_device(&ctx, (uint32_t *)args[0].dev + 8 * GD, (const Fr *)args[1].dev, (const uint32_t *)args[2].dev,
                                            (const uint32_t *)args[3].dev, p.R, p.G, p.e);
    });
    if (run) return run;
    return 0;
}

}  // extern "C"
