// coset_recover_shim.hip -- the device stages of ckzg_hip_recover_cosets_and_kzg_proofs_rows that depend on the coset
// size (coset_recover.hip: the factors of the distinct sets, the per-coset multiplication, the scatter of the held
// cosets) behind a C ABI (tests/test_gpu_coset_recover_stages.py), at every coset size 2^e.  The call reaches them with
// the missing lists of its plan and the `parts` of its picker; here both are the caller's.
//
// Linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libcoset_recover_shim.so), so the kernels are the product's binary
// code; the shim launches no kernel of its own.  The stages need the stream, d_roots and d_shift[2^e] of their
// DeviceCtx and nothing else: the shim makes d_roots from the 8193 powers of w and d_shift from the 7^l the caller
// passes.  Test aid only; its exports are crs_* and none of them is part of libckzg_hip.so.
//
// Calling convention (dev_shim_common.hpp): host pointers in and out, a stream of its own per call, a polling 20 s
// deadline, a non-zero return on any HIP error; what the stage itself returned goes to *rc.  Field elements cross as
// canonical little-endian limbs (8 words), also where the stage holds them in Montgomery form -- such a buffer is
// converted whole, guards included, so what a caller pre-fills it with must be < r.  Every buffer a stage writes goes
// up as the caller filled it with CRS_GUARD elements in front of the data and CRS_GUARD behind, and comes back whole.
#include <cstring>
#include "dev_shim_common.hpp"
#include "device.hpp"
#include "coset_recover_plan.hpp"

using namespace ckzg;
using namespace ckzg::dev;

namespace {

constexpr size_t CRS_GUARD = 64;
constexpr size_t CRS_MAX_SETS = 256, CRS_MAX_ROWS = 64;

std::vector<Fr> fr_in(const uint32_t *raw, size_t n) {
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; i++) v[i] = from_raw<FrParams>(raw + 8 * i);
    return v;
}
void fr_out(uint32_t *raw, const std::vector<Fr> &v) {
    for (size_t i = 0; i < v.size(); i++) to_raw<FrParams>(raw + 8 * i, v[i]);
}
bool size_ok(int e) { return e >= 0 && e <= COSET_RECOVER_MAX_LOG; }

}  // namespace

extern "C" {

static_assert(sizeof(Fr) == 32, "the limbs the tests pass");

size_t crs_guard() { return CRS_GUARD; }

// z_domain, z_coset_inv [G + nsets m + G][8] go up as the caller filled them (values < r); miss_start [nsets + 1], miss
// [miss_start[nsets]]: the root indices (<= 8192) of each set's missing cosets, at most m of them a set; parts: a power
// of two the stage accepts; roots [8193][8]; seven_l [8] = 7^l
int crs_factors(uint32_t *z_domain, uint32_t *z_coset_inv, const uint32_t *miss, const uint32_t *miss_start, size_t nsets, int e,
                uint32_t parts, const uint32_t *roots, const uint32_t *seven_l, int *rc) {
    if (!size_ok(e) || !nsets || nsets > CRS_MAX_SETS || miss_start[0] != 0) return DS_BAD_ARG;
    const size_t G = CRS_GUARD, m = coset_recover_cosets(e);
    for (size_t s = 0; s < nsets; s++)
        if (miss_start[s] > miss_start[s + 1] || miss_start[s + 1] - miss_start[s] > m) return DS_BAD_ARG;
    const size_t total = miss_start[nsets];
    for (size_t i = 0; i < total; i++)
        if (miss[i] > COSET_RECOVER_EXT) return DS_BAD_ARG;
    std::vector<Fr> zd = fr_in(z_domain, nsets * m + 2 * G), zi = fr_in(z_coset_inv, nsets * m + 2 * G);
    const std::vector<Fr> rootv = fr_in(roots, COSET_RECOVER_EXT + 1);
    std::vector<Fr> shiftv(65, Fr::zero());
    shiftv[(size_t)1 << e] = from_raw<FrParams>(seven_l);
    std::vector<Arg> args = {{zd.data(), zd.data(), zd.size() * 32, nullptr},
                             {zi.data(), zi.data(), zi.size() * 32, nullptr},
                             {miss, nullptr, total * 4, nullptr},
                             {miss_start, nullptr, (nsets + 1) * 4, nullptr},
                             {rootv.data(), nullptr, rootv.size() * 32, nullptr},
                             {shiftv.data(), nullptr, shiftv.size() * 32, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        ctx.d_roots = (Fr *)args[4].dev;
        ctx.d_shift = (Fr *)args[5].dev;
        *rc = coset_recover_factors_enqueue(&ctx, (Fr *)args[0].dev + G, (Fr *)args[1].dev + G, (const uint32_t *)args[2].dev,
                                            (const uint32_t *)args[3].dev, nsets, e, parts);
        ctx.d_roots = ctx.d_shift = nullptr;
    });
    if (run) return run;
    fr_out(z_domain, zd);
    fr_out(z_coset_inv, zi);
    return 0;
}

// a [G + 8192 nrows + G][8] goes up as the caller filled it (values < r); f [nsets m][8]; row_set [nrows] < nsets
int crs_mul_factor(uint32_t *a, const uint32_t *f, const uint32_t *row_set, size_t nrows, size_t nsets, int e, int *rc) {
    if (!size_ok(e) || !nrows || nrows > CRS_MAX_ROWS || !nsets || nsets > CRS_MAX_SETS) return DS_BAD_ARG;
    for (size_t r = 0; r < nrows; r++)
        if (row_set[r] >= nsets) return DS_BAD_ARG;
    const size_t G = CRS_GUARD, m = coset_recover_cosets(e);
    std::vector<Fr> av = fr_in(a, nrows * COSET_RECOVER_EXT + 2 * G);
    const std::vector<Fr> fv = fr_in(f, nsets * m);
    std::vector<Arg> args = {{av.data(), av.data(), av.size() * 32, nullptr},
                             {fv.data(), nullptr, fv.size() * 32, nullptr},
                             {row_set, nullptr, nrows * 4, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = fr_mul_coset_factor_enqueue(&ctx, (Fr *)args[0].dev + G, (const Fr *)args[1].dev, (const uint32_t *)args[2].dev,
                                          nrows, e);
    });
    if (run) return run;
    fr_out(a, av);
    return 0;
}

// image [(G + 8192 nrows + G) * 32] bytes goes up as the caller filled it; in [ncosets][32 << e] bytes; coset_dst
// [ncosets] < nrows m
int crs_scatter(uint8_t *image, const uint8_t *in, const uint32_t *coset_dst, size_t ncosets, size_t nrows, int e, int *rc) {
    if (!size_ok(e) || !nrows || nrows > CRS_MAX_ROWS || !ncosets) return DS_BAD_ARG;
    const size_t G = CRS_GUARD, m = coset_recover_cosets(e);
    if (ncosets > nrows * m) return DS_BAD_ARG;
    for (size_t i = 0; i < ncosets; i++)
        if (coset_dst[i] >= nrows * m) return DS_BAD_ARG;
    std::vector<Arg> args = {{image, image, (nrows * COSET_RECOVER_EXT + 2 * G) * 32, nullptr},
                             {in, nullptr, ncosets * ((size_t)32 << e), nullptr},
                             {coset_dst, nullptr, ncosets * 4, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = scatter_cosets_rows_enqueue(&ctx, (uint8_t *)args[0].dev + G * 32, (const uint8_t *)args[1].dev,
                                          (const uint32_t *)args[2].dev, ncosets, e);
    });
}

}  // extern "C"
