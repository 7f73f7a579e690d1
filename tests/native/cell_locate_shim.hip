// cell_locate_shim.hip -- the two stages that the cell form of the *_locate calls adds in front of the point form's
// pipeline, behind a C ABI (tests/test_gpu_cell_locate_stages.py): cell_interp_digits_enqueue (k_cell_interp_digits, and
// its three-pass A/B partner) and the chain interpolation -> 64-term fixed-base sum -> cell_lhs_enqueue (k_cell_lhs).
// The values are read off the device whole, guard included, and compared with integers.
//
// Linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libcell_locate_shim.so), like the stage shim: the kernels it runs
// are the product's binary code.  A bare DeviceCtx is enough: the stream, d_roots, the timing events
// msm_small_vectors_device records.  Test aid only; its exports are cs_* and none of them is part of libckzg_hip.so.
//
// Calling convention (dev_shim_common.hpp): host pointers in and out, a stream of its own per call, a polling 20 s
// deadline, a non-zero return on any HIP error.  Field elements cross as canonical little-endian limbs (8 words);
// points as the device holds them: affine 96 bytes (x | y, Montgomery form, all zero = infinity), XYZZ 192 bytes.
#include "dev_shim_common.hpp"
#include "device.hpp"

using namespace ckzg;
using namespace ckzg::dev;

namespace {

constexpr size_t CS_MAX_CELLS = 4096;   // no call of a test comes near; keeps every buffer small

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

bool geometry(FixedBaseTable &t, int wbits) {
    if (wbits < 2 || wbits > 12) return false;
    call_table_geometry(&t, 64, wbits);
    return true;
}

}  // namespace

extern "C" {

static_assert(sizeof(G1Affine) == 96 && sizeof(G1XYZZ) == 192 && sizeof(Fr) == 32, "the strings the tests pass");

// digits per cell for a window width (2 twin windows of 64 digits), 0 for a width out of range
size_t cs_digits_per_cell(int wbits) {
    FixedBaseTable t;
    return geometry(t, wbits) ? (size_t)t.nwin * 64 : 0;
}

// digits [digits_elems] goes up as the caller filled it: n * cs_digits_per_cell(wbits) digits, then the guard.
// cells [n][64][8]: the cells' field elements, canonical; col [n]; roots: w^i, 8193 of them.  fused = 0: the three-pass form.
int cs_cell_interp_digits(int16_t *digits, size_t digits_elems, const uint32_t *cells, const uint32_t *col, const uint32_t *roots,
                          size_t n, int wbits, int fused) {
    FixedBaseTable t;
    if (!n || n > CS_MAX_CELLS || !geometry(t, wbits) || digits_elems < n * (size_t)t.nwin * 64) return DS_BAD_ARG;
    const size_t npad = (n + 63) / 64 * 64;
    std::vector<Fr> cf = fr_in(cells, n * 64);
    cf.resize(npad * 64, Fr::zero());
    const std::vector<Fr> rootsf = fr_in(roots, 8193);
    std::vector<Arg> args = {{digits, digits, digits_elems * 2, nullptr},
                             {cf.data(), nullptr, cf.size() * 32, nullptr},
                             {col, nullptr, n * 4, nullptr},
                             {rootsf.data(), nullptr, rootsf.size() * 32, nullptr},
                             {nullptr, nullptr, n * 64 * 32, nullptr}};
    int rc = 0;
    const int run = run_bounded(args, [&](hipStream_t st) {
        BareCtx b(st, (Fr *)args[3].dev);
        rc = b.ok ? cell_interp_digits_enqueue(&b.ctx, (int16_t *)args[0].dev, (Fr *)args[1].dev, (const uint32_t *)args[2].dev, n,
                                               t.wbits, t.twin, fused != 0, (uint32_t *)args[4].dev)
                  : DS_BAD_ARG;
    });
    return run ? run : rc;
}

// The chain of a chunk up to its left-hand points, over 64 chosen bases in the place of g1_values_monomial[0..63]:
// table, interpolation digits, the 64-term sums, k_cell_lhs.  pts [n + nc][96]: proofs, then commitments, affine strings
// of the device ((0, 0) = infinity); st_dec, st_sub [n + nc]; commit [n] < nc; cell_bad [n]; mono [64][96].
// lhs [n + 1][192] (XYZZ), neg_proof [n + 1][96] and bad [n + 1] go up as the caller filled them and come back whole:
// the last entry of each is the guard.
int cs_cell_lhs(uint8_t *lhs, uint8_t *neg_proof, uint8_t *bad, const uint8_t *pts, const uint8_t *st_dec, const uint8_t *st_sub,
                const uint32_t *cells, const uint32_t *col, const uint32_t *commit, const uint32_t *cell_bad, const uint8_t *mono,
                const uint32_t *roots, size_t n, size_t nc, int wbits, int fused) {
    FixedBaseTable shape;
    if (!n || n > CS_MAX_CELLS || !nc || nc > n || !geometry(shape, wbits)) return DS_BAD_ARG;
    for (size_t i = 0; i < n; i++)
        if (commit[i] >= nc) return DS_BAD_ARG;
    const size_t npad = (n + 63) / 64 * 64, ndig = n * (size_t)shape.nwin * 64;
    std::vector<Fr> cf = fr_in(cells, n * 64);
    cf.resize(npad * 64, Fr::zero());
    const std::vector<Fr> rootsf = fr_in(roots, 8193);
    std::vector<Arg> args = {{lhs, lhs, (n + 1) * sizeof(G1XYZZ), nullptr},
                             {neg_proof, neg_proof, (n + 1) * sizeof(G1Affine), nullptr},
                             {bad, bad, n + 1, nullptr},
                             {pts, nullptr, (n + nc) * sizeof(G1Affine), nullptr},
                             {st_dec, nullptr, n + nc, nullptr},
                             {st_sub, nullptr, n + nc, nullptr},
                             {cf.data(), nullptr, cf.size() * 32, nullptr},
                             {col, nullptr, n * 4, nullptr},
                             {commit, nullptr, n * 4, nullptr},
                             {cell_bad, nullptr, n * 4, nullptr},
                             {mono, nullptr, 64 * sizeof(G1Affine), nullptr},
                             {rootsf.data(), nullptr, rootsf.size() * 32, nullptr},
                             {nullptr, nullptr, ndig * 2, nullptr},
                             {nullptr, nullptr, n * sizeof(G1XYZZ), nullptr},
                             {nullptr, nullptr, n * 64 * 32, nullptr}};
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
            rc = cell_interp_digits_enqueue(&b.ctx, (int16_t *)args[12].dev, (Fr *)args[6].dev, (const uint32_t *)args[7].dev, n, t.wbits,
                                            t.twin, fused != 0, (uint32_t *)args[14].dev);
        if (!rc) rc = msm_small_vectors_device(&b.ctx, t, (G1XYZZ *)args[13].dev, (const int16_t *)args[12].dev, n, 64, 1);
        if (!rc)
            rc = cell_lhs_enqueue(&b.ctx, (G1XYZZ *)args[0].dev, (G1Affine *)args[1].dev, (uint8_t *)args[2].dev,
                                  (const G1Affine *)args[3].dev, (const uint8_t *)args[4].dev, (const uint8_t *)args[5].dev,
                                  (const G1XYZZ *)args[13].dev, (const uint32_t *)args[7].dev, (const uint32_t *)args[8].dev,
                                  (const uint32_t *)args[9].dev, n);
        // the table goes once nothing reads it any more
        (void)hipStreamSynchronize(st);
        if (t.d_table) (void)hipFree(t.d_table);
    });
    return run ? run : rc;
}

}  // extern "C"
