// coset_repair_shim.hip -- the device stages of ckzg_hip_repair_cosets_and_kzg_proofs_rows (coset_repair.hip: the degree
// flag of a row, the recoding of a row's blob half and its commitment, the comparison of commitments) behind a C ABI
// (tests/test_gpu_coset_repair_stages.py).
//
// Linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libcoset_repair_shim.so), so the kernels are the product's binary
// code; the shim launches no kernel of its own.  Test aid only; its exports are crp_* and none of them is part of
// libckzg_hip.so.
//
// Calling convention (dev_shim_common.hpp): host pointers in and out, a stream of its own per call, a polling 20 s
// deadline, a non-zero return on any HIP error; what the stage itself returned goes to *rc.  Field elements cross as
// canonical little-endian limbs (8 words) and are converted to Montgomery form here.  A buffer a stage writes goes up as
// the caller filled it, CRP_GUARD words (or bytes) in front of the data and CRP_GUARD behind, and comes back whole.
#include <cstring>
#include "dev_shim_common.hpp"
#include "device.hpp"

using namespace ckzg;
using namespace ckzg::dev;

namespace {

constexpr size_t CRP_GUARD = 64, CRP_MAX_ROWS = 16, ROW = 8192;

std::vector<Fr> fr_in(const uint32_t *raw, size_t n) {
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; i++) v[i] = from_raw<FrParams>(raw + 8 * i);
    return v;
}

struct BareCtx {
    DeviceCtx ctx;
    bool ok = true;
    explicit BareCtx(hipStream_t st) {
        ctx.stream = st;
        for (hipEvent_t &e : ctx.ev)
            if (hipEventCreate(&e) != hipSuccess) {
                e = nullptr;
                ok = false;
            }
    }
    ~BareCtx() {
        for (hipEvent_t &e : ctx.ev)
            if (e) (void)hipEventDestroy(e);
        if (ctx.scratch.ptr) (void)hipFree(ctx.scratch.ptr);
        if (ctx.commit.d_table) (void)hipFree(ctx.commit.d_table);
        ctx.commit.d_table = nullptr;
    }
};

}  // namespace

extern "C" {

static_assert(sizeof(Fr) == 32 && sizeof(G1Affine) == 96, "the limbs and points the shim moves");

size_t crp_guard() { return CRP_GUARD; }

// flags [G + nrows + G] words go up as the caller filled them; rows [nrows][8192][8] canonical words
int crp_high_degree(uint32_t *flags, const uint32_t *rows, size_t nrows, int *rc) {
    if (!nrows || nrows > CRP_MAX_ROWS) return DS_BAD_ARG;
    const size_t G = CRP_GUARD;
    const std::vector<Fr> rv = fr_in(rows, nrows * ROW);
    std::vector<Arg> args = {{flags, flags, (nrows + 2 * G) * 4, nullptr}, {rv.data(), nullptr, rv.size() * 32, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = rows_high_degree_enqueue(&ctx, (uint32_t *)args[0].dev + G, (const Fr *)args[1].dev, nrows);
    });
}

// out [G + 48 nrows + G] bytes go up as the caller filled them; rows as above; bases48 [4096][48]: the compressed bases of
// the commitment table, in the table's order, decompressed here and built into a table of window width wbits that is
// installed as ctx->commit for the call
int crp_rows_commit(uint8_t *out, const uint32_t *rows, size_t nrows, const uint8_t *bases48, int wbits, int *rc) {
    if (!nrows || nrows > CRP_MAX_ROWS || wbits < 2 || wbits > 6) return DS_BAD_ARG;
    const size_t G = CRP_GUARD;
    const std::vector<Fr> rv = fr_in(rows, nrows * ROW);
    std::vector<uint8_t> st_host(N_BLOB, 0xff);
    std::vector<Arg> args = {{out, out, nrows * 48 + 2 * G, nullptr},
                             {rv.data(), nullptr, rv.size() * 32, nullptr},
                             {bases48, nullptr, (size_t)N_BLOB * 48, nullptr},
                             {nullptr, nullptr, (size_t)N_BLOB * sizeof(G1Affine), nullptr},
                             {nullptr, st_host.data(), (size_t)N_BLOB, nullptr}};
    int bad_base = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st);
        DeviceCtx &ctx = b.ctx;
        *rc = b.ok ? decompress_g1_batch_device(&ctx, (G1Affine *)args[3].dev, (uint8_t *)args[4].dev, (const uint8_t *)args[2].dev, N_BLOB)
                   : DS_BAD_ARG;
        if (*rc == 0) *rc = build_fixed_base_table(&ctx, &ctx.commit, (const G1Affine *)args[3].dev, N_BLOB, wbits);
        if (*rc == 0) *rc = scratch_reserve(&ctx, commit_scratch_bytes(&ctx, nrows));
        if (*rc == 0) *rc = fr_rows_commit_enqueue(&ctx, (uint8_t *)args[0].dev + G, (const Fr *)args[1].dev, nrows);
        // (the table and the scratch area are freed when b leaves: after the stream has run dry)
        if (hipStreamSynchronize(st) != hipSuccess) *rc = DS_BAD_ARG;
    });
    if (run) return run;
    for (uint8_t f : st_host) bad_base |= f;
    return bad_base ? DS_BAD_ARG : 0;
}

// flags [G + nrows + G] words as above; got, want [nrows][48] bytes
int crp_commit_compare(uint32_t *flags, const uint8_t *got, const uint8_t *want, size_t nrows, int *rc) {
    if (!nrows || nrows > 4096) return DS_BAD_ARG;
    const size_t G = CRP_GUARD;
    std::vector<Arg> args = {{flags, flags, (nrows + 2 * G) * 4, nullptr}, {got, nullptr, nrows * 48, nullptr}, {want, nullptr, nrows * 48, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = commit_compare_enqueue(&ctx, (uint32_t *)args[0].dev + G, (const uint8_t *)args[1].dev, (const uint8_t *)args[2].dev, nrows);
    });
}

}  // extern "C"
