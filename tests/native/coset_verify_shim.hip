// coset_verify_shim.hip -- the device stages of ckzg_hip_verify_coset_kzg_proof_batch (coset_verify.hip: the scalars of
// the combination, the aggregate, the columns' inverse transforms and the fold over the columns) behind a C ABI
// (tests/test_gpu_coset_verify_stages.py), at every coset size 2^e.  The call itself reaches them with the challenge of
// its transcript; here r, the items and their columns are the caller's.
//
// Linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libcoset_verify_shim.so), so the kernels are the product's binary
// code; the shim launches no kernel of its own.  The stages need the stream and d_roots of their DeviceCtx and nothing
// else: the shim makes d_roots from the 8193 powers of w the caller passes.  Test aid only; its exports are cvs_* and
// none of them is part of libckzg_hip.so.
//
// Calling convention (dev_shim_common.hpp): host pointers in and out, a stream of its own per call, a polling 20 s
// deadline, a non-zero return on any HIP error; what the stage itself returned goes to *rc.  Field elements cross as
// canonical little-endian limbs (8 words), also where the stage holds them in Montgomery form -- such a buffer is
// converted whole, guards included, so what a caller pre-fills it with must be < r.  Every buffer a stage writes goes
// up as the caller filled it with CVS_GUARD elements in front of the data and CVS_GUARD behind, and comes back whole.
#include <cstring>
#include "dev_shim_common.hpp"
#include "device.hpp"
#include "coset_verify_plan.hpp"

using namespace ckzg;
using namespace ckzg::dev;

namespace {

constexpr size_t CVS_GUARD = 64;
constexpr size_t CVS_MAX_ITEMS = 1 << 16, CVS_MAX_ELEMS = (size_t)1 << 20;

std::vector<Fr> fr_in(const uint32_t *raw, size_t n) {
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; i++) v[i] = from_raw<FrParams>(raw + 8 * i);
    return v;
}
void fr_out(uint32_t *raw, const std::vector<Fr> &v) {
    for (size_t i = 0; i < v.size(); i++) to_raw<FrParams>(raw + 8 * i, v[i]);
}
bool csr_ok(const uint32_t *start, size_t nrows, const uint32_t *order, size_t n) {
    if (start[0] != 0 || start[nrows] != n) return false;
    for (size_t t = 0; t < nrows; t++)
        if (start[t] > start[t + 1]) return false;
    for (size_t i = 0; i < n; i++)
        if (order[i] >= n) return false;
    return true;
}
bool size_ok(int e) { return e >= 0 && e <= COSET_MAX_LOG; }

}  // namespace

extern "C" {

static_assert(sizeof(Fr) == 32, "the limbs the tests pass");

size_t cvs_guard() { return CVS_GUARD; }

// rp, vec_rp, vec_wrp [G + n + G][8] and vec_w [G + nc + G][8] go up as the caller filled them (rp: values < r);
// coset_idx [n] < 8192 >> e; grp_start [nc + 1], members [n]: the items of each distinct commitment; r [8]; roots [8193][8]
int cvs_rlc_scalars(uint32_t *rp, uint32_t *vec_rp, uint32_t *vec_wrp, uint32_t *vec_w, const uint32_t *coset_idx,
                    const uint32_t *grp_start, const uint32_t *members, const uint32_t *r, const uint32_t *roots, size_t n, size_t nc,
                    int e, int *rc) {
    if (!size_ok(e) || !n || n > CVS_MAX_ITEMS || !nc || nc > n || !csr_ok(grp_start, nc, members, n)) return DS_BAD_ARG;
    for (size_t i = 0; i < n; i++)
        if (coset_idx[i] >= coset_verify_cosets(e)) return DS_BAD_ARG;
    const size_t G = CVS_GUARD;
    std::vector<Fr> rpv = fr_in(rp, n + 2 * G);
    const std::vector<Fr> rootv = fr_in(roots, COSET_VERIFY_EXT + 1);
    const Fr rr = from_raw<FrParams>(r);
    std::vector<Arg> args = {{rpv.data(), rpv.data(), rpv.size() * 32, nullptr},
                             {vec_rp, vec_rp, (n + 2 * G) * 32, nullptr},
                             {vec_wrp, vec_wrp, (n + 2 * G) * 32, nullptr},
                             {vec_w, vec_w, (nc + 2 * G) * 32, nullptr},
                             {coset_idx, nullptr, n * 4, nullptr},
                             {grp_start, nullptr, (nc + 1) * 4, nullptr},
                             {members, nullptr, n * 4, nullptr},
                             {rootv.data(), nullptr, rootv.size() * 32, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        ctx.d_roots = (Fr *)args[7].dev;
        *rc = coset_rlc_scalars_enqueue(&ctx, (Fr *)args[0].dev + G, (uint32_t *)args[1].dev + 8 * G, (uint32_t *)args[2].dev + 8 * G,
                                        (uint32_t *)args[3].dev + 8 * G, (const uint32_t *)args[4].dev, (const uint32_t *)args[5].dev,
                                        (const uint32_t *)args[6].dev, rr, n, nc, e);
    });
    if (run) return run;
    fr_out(rp, rpv);
    return 0;
}

// agg [G + 8192 + G][8] goes up as the caller filled it (values < r); item_fr [n << e][8]; rp [n][8]; col_start
// [(8192 >> e) + 1], order [n]: the items of each coset
int cvs_aggregate(uint32_t *agg, const uint32_t *item_fr, const uint32_t *rp, const uint32_t *col_start, const uint32_t *order,
                  size_t n, int e, int *rc) {
    if (!size_ok(e) || !n || n > CVS_MAX_ITEMS || (n << e) > CVS_MAX_ELEMS) return DS_BAD_ARG;
    if (!csr_ok(col_start, coset_verify_cosets(e), order, n)) return DS_BAD_ARG;
    const size_t G = CVS_GUARD;
    std::vector<Fr> out = fr_in(agg, COSET_VERIFY_EXT + 2 * G);
    const std::vector<Fr> iv = fr_in(item_fr, n << e), rv = fr_in(rp, n);
    std::vector<Arg> args = {{out.data(), out.data(), out.size() * 32, nullptr},
                             {iv.data(), nullptr, iv.size() * 32, nullptr},
                             {rv.data(), nullptr, n * 32, nullptr},
                             {col_start, nullptr, ((size_t)coset_verify_cosets(e) + 1) * 4, nullptr},
                             {order, nullptr, n * 4, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = coset_aggregate_device(&ctx, (Fr *)args[0].dev + G, (const Fr *)args[1].dev, (const Fr *)args[2].dev,
                                     (const uint32_t *)args[3].dev, (const uint32_t *)args[4].dev, n, e);
    });
    if (run) return run;
    fr_out(agg, out);
    return 0;
}

// agg [G + 8192 + G][8] in (the aggregate) and out (each column's coefficients), partial [G + 32 l + G][8] (values < r)
// and interp [G + l + G][8] (canonical, as the stage writes them) go up as the caller filled them; roots [8193][8]
int cvs_interp(uint32_t *interp, uint32_t *partial, uint32_t *agg, const uint32_t *roots, int e, int *rc) {
    if (!size_ok(e)) return DS_BAD_ARG;
    const size_t G = CVS_GUARD, l = (size_t)1 << e;
    std::vector<Fr> av = fr_in(agg, COSET_VERIFY_EXT + 2 * G), pv = fr_in(partial, COSET_INTERP_BLOCKS * l + 2 * G);
    const std::vector<Fr> rootv = fr_in(roots, COSET_VERIFY_EXT + 1);
    std::vector<Arg> args = {{interp, interp, (l + 2 * G) * 32, nullptr},
                             {pv.data(), pv.data(), pv.size() * 32, nullptr},
                             {av.data(), av.data(), av.size() * 32, nullptr},
                             {rootv.data(), nullptr, rootv.size() * 32, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        ctx.d_roots = (Fr *)args[3].dev;
        *rc = coset_interp_device(&ctx, (uint32_t *)args[0].dev + 8 * G, (Fr *)args[1].dev + G, (Fr *)args[2].dev + G, e);
    });
    if (run) return run;
    fr_out(partial, pv);
    fr_out(agg, av);
    return 0;
}

}  // extern "C"
