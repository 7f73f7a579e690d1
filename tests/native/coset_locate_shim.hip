// coset_locate_shim.hip -- the two stages that ckzg_hip_verify_coset_kzg_proof_batch_locate adds in front of the point
// form's pipeline, at every coset size l = 2^e, behind a C ABI (tests/test_gpu_coset_locate_stages.py):
// coset_item_interp_digits_enqueue (k_coset_item_interp_digits) alone, and the chain interpolation -> l-term fixed-base
// sum on a prefix of a 64-point table -> coset_item_lhs_enqueue (k_coset_item_lhs) over caller-chosen bases.  The values
// are read off the device whole, guard included, and compared with integers.  cls_sum_forms times the sum's launch
// forms for tools/bench_coset_locate.py.
//
// Linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libcoset_locate_shim.so), like the cell-locate shim: the kernels it
// runs are the product's binary code.  A bare DeviceCtx is enough: the stream, d_roots, the timing events the sums
// record.  Test aid only; its exports are cls_* and none of them is part of libckzg_hip.so.
//
// Calling convention (dev_shim_common.hpp): host pointers in and out, a stream of its own per call, a polling 20 s
// deadline, a non-zero return on any HIP error.  Field elements cross as canonical little-endian limbs (8 words);
// points as the device holds them: affine 96 bytes (x | y, Montgomery form, all zero = infinity), XYZZ 192 bytes.
#include "dev_shim_common.hpp"
#include "device.hpp"
#include "coset_locate_plan.hpp"

using namespace ckzg;
using namespace ckzg::dev;

namespace {

constexpr size_t CLS_MAX_ITEMS = 16384;   // no call of a test comes near; the timing runs go up to 8,192

std::vector<Fr> fr_in(const uint32_t *raw, size_t n) {
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; i++) v[i] = from_raw<FrParams>(raw + 8 * i);
    return v;
}
// the stream, d_roots and the timing events of a bare context; the events die with it
struct BareCtx {
    DeviceCtx ctx;
    bool ok = true;
    BareCtx(hipStream_t st, Fr *d_roots) {
        ctx.stream = st;
        ctx.d_roots = d_roots;
        for (hipEvent_t &e : ctx.ev)
            if (hipEventCreate(&e) != hipSuccess) {
                e = nullptr;
                ok = false;
            }
    }
    ~BareCtx() {
        for (hipEvent_t &e : ctx.ev)
            if (e) (void)hipEventDestroy(e);
    }
};

bool geometry(FixedBaseTable &t, int wbits, int e) {
    if (wbits < 2 || wbits > 12 || e < 0 || e > COSET_MAX_LOG) return false;
    call_table_geometry(&t, 64, wbits);
    return true;
}

}  // namespace

extern "C" {

static_assert(sizeof(G1Affine) == 96 && sizeof(G1XYZZ) == 192 && sizeof(Fr) == 32, "the strings the tests pass");

// digits per item for a window width and a coset size (2 twin windows of l digits), 0 for arguments out of range
size_t cls_digits_per_item(int wbits, int e) {
    FixedBaseTable t;
    return geometry(t, wbits, e) ? (size_t)t.nwin << e : 0;
}

// the form the product launches the sums in (coset_locate_plan.hpp)
int cls_sum_lpv(int e, uint64_t items) { return e < 0 || e > COSET_MAX_LOG ? 0 : coset_locate_sum_lpv(e, items); }

// digits [digits_elems] goes up as the caller filled it: n * cls_digits_per_item(wbits, e) digits, then the guard.
// vals [n][l][8]: the items' values, canonical; idx [n] (any value: the kernel clamps); roots: w^i, 8193 of them.
int cls_coset_interp_digits(int16_t *digits, size_t digits_elems, const uint32_t *vals, const uint32_t *idx, const uint32_t *roots,
                            size_t n, int e, int wbits) {
    FixedBaseTable t;
    if (!n || n > CLS_MAX_ITEMS || !geometry(t, wbits, e) || digits_elems < (n * (size_t)t.nwin << e)) return DS_BAD_ARG;
    const std::vector<Fr> vf = fr_in(vals, n << e);
    const std::vector<Fr> rootsf = fr_in(roots, 8193);
    std::vector<Arg> args = {{digits, digits, digits_elems * 2, nullptr},
                             {vf.data(), nullptr, vf.size() * 32, nullptr},
                             {idx, nullptr, n * 4, nullptr},
                             {rootsf.data(), nullptr, rootsf.size() * 32, nullptr}};
    int rc = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st, (Fr *)args[3].dev);
        rc = b.ok ? coset_item_interp_digits_enqueue(&b.ctx, (int16_t *)args[0].dev, (const Fr *)args[1].dev,
                                                     (const uint32_t *)args[2].dev, n, e, t.wbits, t.twin)
                  : DS_BAD_ARG;
    });
    return run ? run : rc;
}

// The chain of a chunk up to its left-hand points, over 64 chosen bases in the place of g1_values_monomial[0..63]: the
// 64-point table, interpolation digits, the l-term sums on the table's prefix (lpv lanes per vector; 0: the product's
// choice for (e, n)), k_coset_item_lhs.  pts [n + nc][96]: proofs, then commitments, affine strings of the device
// ((0, 0) = infinity); st_dec, st_sub [n + nc]; commit [n] < nc; val_bad [n]; mono [64][96].
// lhs [n + 1][192] (XYZZ), neg_proof [n + 1][96] and bad [n + 1] go up as the caller filled them and come back whole:
// the last entry of each is the guard.
int cls_coset_lhs(uint8_t *lhs, uint8_t *neg_proof, uint8_t *bad, const uint8_t *pts, const uint8_t *st_dec, const uint8_t *st_sub,
                  const uint32_t *vals, const uint32_t *idx, const uint32_t *commit, const uint32_t *val_bad, const uint8_t *mono,
                  const uint32_t *roots, size_t n, size_t nc, int e, int wbits, int lpv) {
    FixedBaseTable shape;
    if (!n || n > CLS_MAX_ITEMS || !nc || nc > n || !geometry(shape, wbits, e)) return DS_BAD_ARG;
    if (lpv != 0 && lpv != 4 && lpv != 8 && lpv != 16 && lpv != 64) return DS_BAD_ARG;
    for (size_t i = 0; i < n; i++)
        if (commit[i] >= nc) return DS_BAD_ARG;
    const size_t ndig = n * (size_t)shape.nwin << e;
    const std::vector<Fr> vf = fr_in(vals, n << e);
    const std::vector<Fr> rootsf = fr_in(roots, 8193);
    std::vector<Arg> args = {{lhs, lhs, (n + 1) * sizeof(G1XYZZ), nullptr},
                             {neg_proof, neg_proof, (n + 1) * sizeof(G1Affine), nullptr},
                             {bad, bad, n + 1, nullptr},
                             {pts, nullptr, (n + nc) * sizeof(G1Affine), nullptr},
                             {st_dec, nullptr, n + nc, nullptr},
                             {st_sub, nullptr, n + nc, nullptr},
                             {vf.data(), nullptr, vf.size() * 32, nullptr},
                             {idx, nullptr, n * 4, nullptr},
                             {commit, nullptr, n * 4, nullptr},
                             {val_bad, nullptr, n * 4, nullptr},
                             {mono, nullptr, 64 * sizeof(G1Affine), nullptr},
                             {rootsf.data(), nullptr, rootsf.size() * 32, nullptr},
                             {nullptr, nullptr, ndig * 2, nullptr},
                             {nullptr, nullptr, n * sizeof(G1XYZZ), nullptr}};
    int rc = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st, (Fr *)args[11].dev);
        if (!b.ok) {
            rc = DS_BAD_ARG;
            return;
        }
        FixedBaseTable t;
        rc = build_fixed_base_table(&b.ctx, &t, (const G1Affine *)args[10].dev, 64, wbits);
        if (!rc)
            rc = coset_item_interp_digits_enqueue(&b.ctx, (int16_t *)args[12].dev, (const Fr *)args[6].dev,
                                                  (const uint32_t *)args[7].dev, n, e, t.wbits, t.twin);
        if (!rc)
            rc = msm_small_vectors_lpv_device(&b.ctx, t, (G1XYZZ *)args[13].dev, (const int16_t *)args[12].dev, n, 1u << e, 1,
                                              lpv ? lpv : coset_locate_sum_lpv(e, n));
        if (!rc)
            rc = coset_item_lhs_enqueue(&b.ctx, (G1XYZZ *)args[0].dev, (G1Affine *)args[1].dev, (uint8_t *)args[2].dev,
                                        (const G1Affine *)args[3].dev, (const uint8_t *)args[4].dev, (const uint8_t *)args[5].dev,
                                        (const G1XYZZ *)args[13].dev, (const uint32_t *)args[7].dev, (const uint32_t *)args[8].dev,
                                        (const uint32_t *)args[9].dev, n, e);
        // the table goes once nothing reads it any more
        (void)hipStreamSynchronize(st);
        if (t.d_table) (void)hipFree(t.d_table);
    });
    return run ? run : rc;
}

// Measurement aid (tools/bench_coset_locate.py --sum-forms): the l-term sums of n items in the form lpv, `reps` launches
// (at most 64) timed one by one between events, after one untimed launch.  ms [reps] <- the launches' times.  Values,
// indices, bases and roots as in cls_coset_lhs.
int cls_sum_forms(float *ms, const uint32_t *vals, const uint32_t *idx, const uint8_t *mono, const uint32_t *roots, size_t n, int e,
                  int wbits, int lpv, int reps) {
    FixedBaseTable shape;
    if (!n || n > CLS_MAX_ITEMS || !geometry(shape, wbits, e) || reps < 1 || reps > 64) return DS_BAD_ARG;
    if (lpv != 4 && lpv != 8 && lpv != 16 && lpv != 64) return DS_BAD_ARG;
    const size_t ndig = n * (size_t)shape.nwin << e;
    const std::vector<Fr> vf = fr_in(vals, n << e);
    const std::vector<Fr> rootsf = fr_in(roots, 8193);
    std::vector<Arg> args = {{vf.data(), nullptr, vf.size() * 32, nullptr},
                             {idx, nullptr, n * 4, nullptr},
                             {mono, nullptr, 64 * sizeof(G1Affine), nullptr},
                             {rootsf.data(), nullptr, rootsf.size() * 32, nullptr},
                             {nullptr, nullptr, ndig * 2, nullptr},
                             {nullptr, nullptr, n * sizeof(G1XYZZ), nullptr}};
    if (hipSetDevice(pick_device()) != hipSuccess) return DS_BAD_ARG;
    std::vector<hipEvent_t> evs(2 * (size_t)reps, nullptr);
    int rc = 0;
    for (hipEvent_t &ev : evs)
        if (hipEventCreate(&ev) != hipSuccess) {
            ev = nullptr;
            rc = DS_BAD_ARG;
        }
    int run = 0;
    if (!rc)
        run = run_bounded(args, [&](hipStream_t st) {
            BareCtx b(st, (Fr *)args[3].dev);
            if (!b.ok) {
                rc = DS_BAD_ARG;
                return;
            }
            FixedBaseTable t;
            rc = build_fixed_base_table(&b.ctx, &t, (const G1Affine *)args[2].dev, 64, wbits);
            if (!rc)
                rc = coset_item_interp_digits_enqueue(&b.ctx, (int16_t *)args[4].dev, (const Fr *)args[0].dev,
                                                      (const uint32_t *)args[1].dev, n, e, t.wbits, t.twin);
            for (int i = -1; i < reps && !rc; i++) {
                if (i >= 0 && hipEventRecord(evs[2 * i], st) != hipSuccess) rc = DS_BAD_ARG;
                if (!rc) rc = msm_small_vectors_lpv_device(&b.ctx, t, (G1XYZZ *)args[5].dev, (const int16_t *)args[4].dev, n, 1u << e, 1, lpv);
                if (!rc && i >= 0 && hipEventRecord(evs[2 * i + 1], st) != hipSuccess) rc = DS_BAD_ARG;
            }
            (void)hipStreamSynchronize(st);
            if (t.d_table) (void)hipFree(t.d_table);
        });
    if (!rc && !run)
        for (int i = 0; i < reps; i++)
            if (hipEventElapsedTime(&ms[i], evs[2 * i], evs[2 * i + 1]) != hipSuccess) rc = DS_BAD_ARG;
    for (hipEvent_t ev : evs)
        if (ev) (void)hipEventDestroy(ev);
    return run ? run : rc;
}

}  // extern "C"
