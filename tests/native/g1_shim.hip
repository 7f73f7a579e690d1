// g1_shim.hip -- the stages that add up G1 points, behind a C ABI (tests/test_gpu_g1_stages.py):
//   msm.hip        build_fixed_base_table (k_window_bases_quad, k_batch_to_affine<to392>, k_table_seeds, k_table_steps),
//                  msm_from_digits_device (k_msm_accumulate<256, RAW>, the five folds of run_msm), msm_small_vectors_device
//                  (k_msm_small<LPV>), commit_blobs_enqueue / msm_commit_table_raw_device (k_blob_digits, k_raw_digits),
//                  call_table_enqueue + table_sums_enqueue (the X28 table, k_raw_digits_n, k_msm_accumulate_x28,
//                  k_msm_reduce_partials), batch_to_affine_device
//   verify.hip     lincomb_multi_device (both lane forms, k_lincomb_final)
//   pippenger.hip  bucket_msm_enqueue
//   locate.hip     g1_prefix_scan_enqueue
// The entry points reach these stages with the trusted setup as bases and with honest points; here the bases, the digit
// vectors and the job layouts are the caller's, so every quantity is a known multiple of the generator.
//
// This file is linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libg1_shim.so), so every kernel is the product's binary
// code, not a second compilation; the shim launches no kernel of its own.  A stage needs `stream` and the timing events
// of its DeviceCtx (run_msm and msm_small_vectors_device record them) and nothing else: no trusted setup.  Test aid only;
// its exports are gs_* and none of them is part of libckzg_hip.so.
//
// Calling convention (dev_shim_common.hpp): host pointers in and out, a stream of its own per call, a polling 20 s
// deadline, a non-zero return on any HIP error.  What the stage itself returned goes to *rc (a refusal is a result, not
// a failure of the call).  Field elements cross as the twelve words the device holds: affine points (96 bytes) and XYZZ
// points (192 bytes) in the 2^384 Montgomery domain, table entries as tb_store_point writes them.  The shim owns all
// device memory of a call and frees it on every path.  Every output buffer goes up as the caller filled it -- data, then
// a guard region the stage is not told about -- and all of it comes back.  What would make a kernel read outside a
// buffer (a digit beyond the table's half, an offset list out of order) is refused here with DS_BAD_ARG.
#include <cstring>
#include "dev_shim_common.hpp"
#include "device.hpp"

using namespace ckzg;
using namespace ckzg::dev;

namespace ckzg {
namespace dev {
// msm.hip: what pick_pairs_per_block(_fixed) returns (no product code outside msm.hip asks, so no header declares it)
uint32_t msm_pairs_per_block(size_t nvec, uint32_t pairs_per_vec, bool fixed);
}  // namespace dev
}  // namespace ckzg

namespace {

constexpr size_t GS_MAX_BYTES = (size_t)3 << 30;   // of one buffer: no call of a test comes near

// geometry only (FixedBaseTable of build_fixed_base_table and of call_table_geometry are the same fields)
bool geometry(FixedBaseTable &t, int npoints, int wbits) {
    if (npoints <= 0 || npoints > (1 << 16) || wbits < 2 || wbits > 16) return false;
    call_table_geometry(&t, npoints, wbits);
    return true;
}

bool digits_ok(const int16_t *d, size_t n, size_t half) {
    for (size_t i = 0; i < n; i++) {
        const int v = d[i];
        if ((size_t)(v < 0 ? -v : v) > half) return false;
    }
    return true;
}

bool offsets_ok(const uint32_t *off, int n, size_t limit) {
    if (off[0] != 0) return false;
    for (int j = 0; j < n; j++)
        if (off[j] > off[j + 1]) return false;
    return off[n] <= limit;
}

// the stream and the timing events of a bare context; the events die with it
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
    }
};

}  // namespace

extern "C" {

static_assert(sizeof(G1Affine) == 96 && sizeof(G1XYZZ) == 192 && sizeof(Fp) == 48, "the strings the tests pass");

// which launch shape run_msm (fixed = 1: msm_from_digits_device, the commitment calls) or table_sums_enqueue (fixed = 0)
// takes for nvec vectors over this table
int gs_msm_plan(int npoints, int wbits, size_t nvec, int fixed, uint32_t *ppb, uint32_t *bpv) {
    FixedBaseTable t;
    if (!geometry(t, npoints, wbits)) return DS_BAD_ARG;
    const uint32_t pairs_per_vec = (uint32_t)t.nwin * t.npoints;
    *ppb = msm_pairs_per_block(nvec, pairs_per_vec, fixed != 0);
    *bpv = (pairs_per_vec + *ppb - 1) / *ppb;
    return 0;
}

// table [table_bytes] goes up as the caller filled it: twin * npoints * half entries, then the guard; bases [npoints][96]
int gs_build_table(uint8_t *table, size_t table_bytes, const uint8_t *bases, int npoints, int wbits, int *rc) {
    if (npoints <= 0 || npoints > (1 << 16) || table_bytes > GS_MAX_BYTES) return DS_BAD_ARG;
    FixedBaseTable shape;
    if (geometry(shape, npoints, wbits) && shape.bytes() > table_bytes) return DS_BAD_ARG;
    std::vector<Arg> args = {{table, table, table_bytes, nullptr}, {bases, nullptr, (size_t)npoints * sizeof(G1Affine), nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st);
        FixedBaseTable t;
        // build_fixed_base_table allocates its table itself.  A block of the same size, filled with the guard's pattern
        // and freed, goes first: the allocator hands the next request of that size the same memory, so an entry the
        // builders never write comes back as the pattern and not as the zeros (= infinity) of fresh memory.
        if (geometry(t, npoints, wbits)) {
            void *dirty = nullptr;
            if (hipMalloc(&dirty, t.bytes()) == hipSuccess) {
                (void)hipMemsetAsync(dirty, 0xa5, t.bytes(), st);
                (void)hipStreamSynchronize(st);
                (void)hipFree(dirty);
            }
        }
        *rc = b.ok ? build_fixed_base_table(&b.ctx, &t, (const G1Affine *)args[1].dev, npoints, wbits) : DS_BAD_ARG;
        if (*rc == 0 && t.d_table) {
            if (hipMemcpyAsync(args[0].dev, t.d_table, t.bytes(), hipMemcpyDeviceToDevice, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                *rc = DS_BAD_ARG;
        }
        if (t.d_table) (void)hipFree(t.d_table);
    });
}

// out [out_bytes] goes up as the caller filled it: nvec * 48 bytes, then the guard; table: what gs_build_table returned
// (table_bytes = 0: no table); digits [nvec][nwin][npoints]
int gs_msm_from_digits(uint8_t *out, size_t out_bytes, const uint8_t *table, size_t table_bytes, int npoints, int wbits,
                       const int16_t *digits, size_t nvec, int *rc) {
    FixedBaseTable t;
    if (!geometry(t, npoints, wbits) || nvec > ((size_t)1 << 16) || out_bytes < nvec * 48 || out_bytes > GS_MAX_BYTES) return DS_BAD_ARG;
    if (table_bytes && table_bytes < t.bytes()) return DS_BAD_ARG;
    const size_t ndig = nvec * (size_t)t.nwin * t.npoints;
    if (ndig * 2 > GS_MAX_BYTES || !digits_ok(digits, ndig, t.half)) return DS_BAD_ARG;
    std::vector<Arg> args = {{out, out, out_bytes, nullptr},
                             {table, nullptr, table_bytes, nullptr},
                             {digits, nullptr, ndig * 2, nullptr},
                             {nullptr, nullptr, msm_partials_needed(t, nvec) * sizeof(G1XYZZ), nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st);
        t.d_table = table_bytes ? (G1Affine *)args[1].dev : nullptr;
        *rc = b.ok ? msm_from_digits_device(&b.ctx, t, (uint8_t *)args[0].dev, (const int16_t *)args[2].dev, (G1XYZZ *)args[3].dev, nvec)
                   : DS_BAD_ARG;
    });
}

// out [out_pts][192] goes up as the caller filled it: nvec sums, then the guard; digits [nvec][nwin][ppv]; vector v
// sums over the points (v % vecs_per_group) * ppv .. + ppv of the table
int gs_msm_small(uint8_t *out, size_t out_pts, const uint8_t *table, size_t table_bytes, int npoints, int wbits,
                 const int16_t *digits, size_t nvec, uint32_t ppv, uint32_t vecs_per_group, int *rc) {
    FixedBaseTable t;
    if (!geometry(t, npoints, wbits) || nvec > ((size_t)1 << 17) || out_pts < nvec || out_pts * sizeof(G1XYZZ) > GS_MAX_BYTES) return DS_BAD_ARG;
    if (table_bytes < t.bytes() || !ppv || !vecs_per_group || (size_t)ppv * vecs_per_group > (size_t)npoints) return DS_BAD_ARG;
    const size_t ndig = nvec * (size_t)t.nwin * ppv;
    if (ndig * 2 > GS_MAX_BYTES || !digits_ok(digits, ndig, t.half)) return DS_BAD_ARG;
    std::vector<Arg> args = {{out, out, out_pts * sizeof(G1XYZZ), nullptr}, {table, nullptr, table_bytes, nullptr}, {digits, nullptr, ndig * 2, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st);
        t.d_table = (G1Affine *)args[1].dev;
        *rc = b.ok ? msm_small_vectors_device(&b.ctx, t, (G1XYZZ *)args[0].dev, (const int16_t *)args[2].dev, nvec, ppv, vecs_per_group)
                   : DS_BAD_ARG;
    });
}

// The commitment calls over a table of 4096 chosen bases, built here and installed as ctx->commit.
//   raw = 0  commit_blobs_enqueue: in = blobs [n][131072], status [n + 1] goes up as the caller filled it
//   raw = 1  msm_commit_table_raw_device: in = scalars [n][4096][8] (canonical words); status is left alone
// out [out_bytes]: n * 48 bytes and the guard, as the caller filled it; digits [n][nwin][4096]: what the call left at the
// head of ctx->scratch
static int gs_commit(uint8_t *out, size_t out_bytes, uint8_t *status, int16_t *digits, const uint8_t *bases, int wbits,
                     const void *in, size_t n, int raw, int *rc) {
    FixedBaseTable shape;
    if (!geometry(shape, N_BLOB, wbits) || !n || n > 64 || out_bytes < n * 48 || shape.bytes() > GS_MAX_BYTES) return DS_BAD_ARG;
    const size_t ndig = n * (size_t)shape.nwin * N_BLOB;
    std::vector<Arg> args = {{out, out, out_bytes, nullptr},
                             {status, status, n + 1, nullptr},
                             {bases, nullptr, (size_t)N_BLOB * sizeof(G1Affine), nullptr},
                             {in, nullptr, raw ? n * N_BLOB * 32 : n * (size_t)N_BLOB * 32, nullptr},
                             {nullptr, digits, ndig * 2, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st);
        DeviceCtx &ctx = b.ctx;
        *rc = b.ok ? build_fixed_base_table(&ctx, &ctx.commit, (const G1Affine *)args[2].dev, N_BLOB, wbits) : DS_BAD_ARG;
        if (*rc == 0) {
            if (raw) {
                *rc = msm_commit_table_raw_device(&ctx, (uint8_t *)args[0].dev, (const uint32_t *)args[3].dev, n);
            } else {
                *rc = scratch_reserve(&ctx, commit_scratch_bytes(&ctx, n));
                if (*rc == 0) *rc = commit_blobs_enqueue(&ctx, (uint8_t *)args[0].dev, (uint8_t *)args[1].dev, (const uint8_t *)args[3].dev, n);
            }
        }
        if (*rc == 0 && (hipMemcpyAsync(args[4].dev, ctx.scratch.ptr, ndig * 2, hipMemcpyDeviceToDevice, st) != hipSuccess ||
                         hipStreamSynchronize(st) != hipSuccess))
            *rc = DS_BAD_ARG;
        if (ctx.commit.d_table) (void)hipFree(ctx.commit.d_table);
        ctx.commit.d_table = nullptr;
    });
}
int gs_commit_blobs(uint8_t *out, size_t out_bytes, uint8_t *status, int16_t *digits, const uint8_t *bases, int wbits,
                    const uint8_t *blobs, size_t n, int *rc) {
    return gs_commit(out, out_bytes, status, digits, bases, wbits, blobs, n, 0, rc);
}
int gs_commit_raw(uint8_t *out, size_t out_bytes, int16_t *digits, const uint8_t *bases, int wbits, const uint32_t *scalars,
                  size_t n, int *rc) {
    uint8_t unused[65] = {};
    return gs_commit(out, out_bytes, unused, digits, bases, wbits, scalars, n, 1, rc);
}

// sums [out_pts][192] goes up as the caller filled it: nvec sums, then the guard; digits [nvec][nwin][npoints]: what
// table_sums_enqueue left at the head of its scratch; points [npoints][96]; scalars [nvec][npoints][8] (canonical words).
// build = 0: the table is never built (table_sums_enqueue must refuse) -- unless x28_table is given: twin * npoints *
// half entries of 4 x 14 limbs made by the caller, which then stand for the table (an entry in a representation the
// builders do not happen to produce)
int gs_table_sums(uint8_t *sums, size_t out_pts, int16_t *digits, const uint8_t *points, int npoints, int wbits,
                  const uint32_t *scalars, size_t nvec, int build, const uint8_t *x28_table, int *rc) {
    FixedBaseTable t;
    if (!geometry(t, npoints, wbits) || wbits > 8 || npoints > 4096 || nvec > 16 || out_pts < nvec || out_pts > 64) return DS_BAD_ARG;
    const size_t ndig = nvec * (size_t)t.nwin * t.npoints;
    std::vector<uint8_t> scratch_host(nvec ? table_sums_scratch_bytes(t, nvec) : 4);
    std::vector<Arg> args = {{sums, sums, out_pts * sizeof(G1XYZZ), nullptr},
                             {points, nullptr, (size_t)npoints * sizeof(G1Affine), nullptr},
                             {scalars, nullptr, nvec * (size_t)npoints * 32, nullptr},
                             {x28_table, nullptr, call_table_bytes(t), nullptr},
                             {nullptr, nullptr, call_table_tmp_bytes(t), nullptr},
                             {nullptr, scratch_host.data(), scratch_host.size(), nullptr}};
    if (build && x28_table) return DS_BAD_ARG;
    const int run = run_bounded(args, [&](hipStream_t st) {
        *rc = build ? call_table_enqueue(st, &t, args[3].dev, (uint8_t *)args[4].dev, (const G1Affine *)args[1].dev) : 0;
        if (x28_table) t.d_table = static_cast<G1Affine *>(args[3].dev);
        if (*rc == 0)
            *rc = table_sums_enqueue(st, t, (G1XYZZ *)args[0].dev, (const uint32_t *)args[2].dev, nvec, (uint8_t *)args[5].dev);
    });
    if (run) return run;
    if (ndig) memcpy(digits, scratch_host.data(), ndig * 2);
    return 0;
}

// out [out_pts][96] goes up as the caller filled it: n points, then the guard; in [n][192]
int gs_batch_to_affine(uint8_t *out, size_t out_pts, const uint8_t *in, size_t n, int *rc) {
    if (out_pts < n || out_pts > ((size_t)1 << 21)) return DS_BAD_ARG;
    std::vector<Arg> args = {{out, out, out_pts * sizeof(G1Affine), nullptr}, {in, nullptr, n * sizeof(G1XYZZ), nullptr}, {nullptr, nullptr, n * sizeof(Fp), nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st);
        *rc = batch_to_affine_device(&b.ctx, (G1Affine *)args[0].dev, (const G1XYZZ *)args[1].dev, (Fp *)args[2].dev, n);
    });
}

// out [njobs + 1][96] goes up as the caller filled it; pts [total][96], scalars [total][8]: the jobs back to back, each
// padded to a multiple of 64 terms with infinity and zero scalars (the layout gpu_lincomb_multi makes); part_off
// [njobs + 1] in partials of 32 terms (quad = 0) or 8 terms (quad = 1)
int gs_lincomb_multi(uint8_t *out, const uint8_t *pts, const uint32_t *scalars, size_t total, const uint32_t *part_off, int njobs,
                     int quad, int *rc) {
    if (njobs <= 0 || njobs > 64 || !total || total % 64 || total > ((size_t)1 << 16)) return DS_BAD_ARG;
    const size_t nparts = total / (quad ? 8 : 32);
    if (!offsets_ok(part_off, njobs, nparts)) return DS_BAD_ARG;
    std::vector<Arg> args = {{out, out, (size_t)(njobs + 1) * sizeof(G1Affine), nullptr},
                             {pts, nullptr, total * sizeof(G1Affine), nullptr},
                             {scalars, nullptr, total * 32, nullptr},
                             {nullptr, nullptr, nparts * sizeof(G1XYZZ), nullptr},
                             {nullptr, nullptr, (size_t)(njobs + 1) * 4, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st);
        *rc = lincomb_multi_device(&b.ctx, (G1Affine *)args[0].dev, (G1XYZZ *)args[3].dev, (uint32_t *)args[4].dev,
                                   (const G1Affine *)args[1].dev, (const uint32_t *)args[2].dev, total, part_off, njobs, quad != 0);
    });
}

// out [njobs + 1][96] goes up as the caller filled it; pts [total][96], scalars [total][8]; job_off [njobs + 1] in terms
int gs_bucket_msm(uint8_t *out, const uint8_t *pts, const uint32_t *scalars, size_t total, const uint32_t *job_off, int njobs,
                  int wbits, int *rc) {
    if (njobs <= 0 || njobs > 64 || !total || total > ((size_t)1 << 16)) return DS_BAD_ARG;
    if (!offsets_ok(job_off, njobs, total)) return DS_BAD_ARG;
    const bool in_range = wbits >= 4 && wbits <= 16;   // (what bucket_msm_enqueue states; outside it nothing is launched)
    if (in_range && wbits > 10) return DS_BAD_ARG;     // keeps the bucket arrays small
    std::vector<Arg> args = {{out, out, (size_t)(njobs + 1) * sizeof(G1Affine), nullptr},
                             {pts, nullptr, total * sizeof(G1Affine), nullptr},
                             {scalars, nullptr, total * 32, nullptr},
                             {nullptr, nullptr, in_range ? bucket_msm_scratch_bytes(total, njobs, wbits) : 4, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st);
        *rc = bucket_msm_enqueue(&b.ctx, (G1Affine *)args[0].dev, (const G1Affine *)args[1].dev, (const uint32_t *)args[2].dev, total,
                                 job_off, njobs, wbits, (uint8_t *)args[3].dev);
    });
}

// data [data_pts][192] in place: nseg arrays of n points, then the guard
int gs_prefix_scan(uint8_t *data, size_t data_pts, size_t n, size_t nseg, int *rc) {
    if (!n || !nseg || nseg > 8 || n > ((size_t)1 << 20) || data_pts < n * nseg || data_pts > ((size_t)1 << 22)) return DS_BAD_ARG;
    std::vector<Arg> args = {{data, data, data_pts * sizeof(G1XYZZ), nullptr},
                             {nullptr, nullptr, g1_prefix_scan_scratch_points(n, nseg) * sizeof(G1XYZZ), nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st);
        *rc = g1_prefix_scan_enqueue(&b.ctx, (G1XYZZ *)args[0].dev, (G1XYZZ *)args[1].dev, n, nseg);
    });
}

}  // extern "C"
