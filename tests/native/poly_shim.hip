// poly_shim.hip -- the stages that move and combine vectors of Fr, behind a C ABI (tests/test_gpu_poly_stages.py):
//   ntt.hip     fr_ntt_batch, bytes_to_fr_batch, fr_to_bytes_batch, zero_extend_batch
//   verify.hip  eval_blob_bytes_batch_device (k_eval_tree), eval_quotient_batch_device (k_eval_barycentric<true>,
//               k_quotient_in_domain), fr_mul_inplace_device, fr_div_inplace_device, scatter_cells_device
//   coset_groups.hip  coset_group_aggregate_device, coset_group_interp_device, coset_group_interp_sum_device at cosets
//               of 64: the aggregation and interpolation of a chunk of cell groups
//   coset_recover.hip  coset_recover_factors_enqueue, fr_mul_coset_factor_enqueue, scatter_cosets_rows_enqueue at cosets
//               of 64: the factors, the multiplication and the scatter of recovery by rows, in the cell call's terms
//   coset_verify.hip  coset_aggregate_device, coset_interp_device at cosets of 64: the aggregation and interpolation of a
//               single cell batch
// They sit between the arithmetic that tests/test_gpu_fields.py pins and the entry points that are compared with the
// oracle, and the entry points reach them with a handful of shapes and with inputs nobody chooses (a hashed z, a
// divisor that is never zero).  Here each one runs on chosen inputs and its whole output comes back.
//
// This file is linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libpoly_shim.so), so every kernel is the product's
// binary code, not a second compilation; the shim has no kernel of its own (ps_eval_blob_bytes replicates its few
// distinct blobs with device-to-device copies).  A stage needs `stream` and the Fr tables of its DeviceCtx and nothing
// else: the shim makes d_roots, d_brp_roots and d_shift from the 8193 powers of w the caller passes, and
// d_brp_roots29 with the product's roots29_build.  No trusted setup.  Test aid only; its exports are ps_* and none of
// them is part of libckzg_hip.so.
//
// Calling convention (dev_shim_common.hpp): host pointers in and out, a stream of its own per call, a polling 20 s
// deadline, a non-zero return on any HIP error.  What the stage itself returned goes to *rc (a refusal is a result,
// not a failure of the call).  Field elements cross as canonical little-endian limbs (8 words), also where the stage
// holds them in Montgomery form -- a buffer of those is converted whole, guard included, so what a caller pre-fills it
// with must be < r; blobs and cells cross as the bytes they are.  Every output buffer comes back whole: where a stage
// works in place or writes part of a buffer, the caller's pre-filled buffer goes up with a guard region behind the
// data (one more tile / run / row than the stage is told about) and all of it comes back.
#include <cstring>
#include "dev_shim_common.hpp"
#include "device.hpp"
#include "coset_recover_plan.hpp"
#include "coset_verify_plan.hpp"

using namespace ckzg;
using namespace ckzg::dev;

namespace {

constexpr int CELL_LOG = 6;   // a cell is a coset of 64 values
constexpr size_t PS_MAX_ELEMS = (size_t)1 << 22;   // field elements of one buffer: no call of a test comes near
constexpr size_t BLOB_BYTES = (size_t)N_BLOB * 32, CELL_BYTES = (size_t)N_CELL * 32;

std::vector<Fr> fr_in(const uint32_t *raw, size_t n) {
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; i++) v[i] = from_raw<FrParams>(raw + 8 * i);
    return v;
}
void fr_out(uint32_t *raw, const std::vector<Fr> &v) {
    for (size_t i = 0; i < v.size(); i++) to_raw<FrParams>(raw + 8 * i, v[i]);
}
uint32_t brp13(uint32_t i) {
    uint32_t o = 0;
    for (int b = 0; b < 13; b++) o |= ((i >> b) & 1u) << (12 - b);
    return o;
}

// the Fr tables of a DeviceCtx, from w^i, i <= 8192
struct Tables {
    std::vector<Fr> roots, brp, shift;
    explicit Tables(const uint32_t *roots_raw) : roots(fr_in(roots_raw, N_EXT + 1)), brp(N_EXT), shift(N_EXT) {
        for (uint32_t i = 0; i < (uint32_t)N_EXT; i++) brp[i] = roots[brp13(i)];
        const uint32_t seven_raw[8] = {7, 0, 0, 0, 0, 0, 0, 0};
        const Fr seven = from_raw<FrParams>(seven_raw);
        shift[0] = Fr::one();
        for (int i = 1; i < N_EXT; i++) shift[i] = mul(shift[i - 1], seven);
    }
    // appends roots | brp_roots | shift | roots29 to the arguments; returns the index of the first
    size_t push(std::vector<Arg> &args) const {
        const size_t at = args.size();
        args.push_back({roots.data(), nullptr, roots.size() * sizeof(Fr), nullptr});
        args.push_back({brp.data(), nullptr, brp.size() * sizeof(Fr), nullptr});
        args.push_back({shift.data(), nullptr, shift.size() * sizeof(Fr), nullptr});
        args.push_back({nullptr, nullptr, (size_t)ROOTS29_ENTRIES * 9 * sizeof(uint32_t), nullptr});
        return at;
    }
};

// all a stage function reads of its context; d_brp_roots29 by the product's own kernel, on the same stream
int stage_ctx(DeviceCtx &ctx, hipStream_t st, const std::vector<Arg> &args, size_t at) {
    ctx.stream = st;
    ctx.d_roots = (Fr *)args[at].dev;
    ctx.d_brp_roots = (Fr *)args[at + 1].dev;
    ctx.d_shift = (Fr *)args[at + 2].dev;
    ctx.d_brp_roots29 = (uint32_t *)args[at + 3].dev;
    return roots29_build(&ctx, ctx.d_brp_roots29);
}

// rows of 64 coefficients -> each row's values over the 64th roots of unity, in bit-reversed order, on the host:
// value j = sum_k coeffs[k] w_64^(brp_6(j) k), w_64 = w^128
std::vector<Fr> values_of_coeffs64(const Tables &tb, const std::vector<Fr> &coeffs) {
    std::vector<Fr> values(coeffs.size());
    for (size_t c = 0; c < coeffs.size() / 64; c++) {
        for (uint32_t j = 0; j < 64; j++) {
            const uint32_t t = brp13(j) >> 7;   // brp_6(j)
            Fr acc = Fr::zero();
            for (uint32_t k = 0; k < 64; k++) acc = add(acc, mul(coeffs[c * 64 + k], tb.roots[(128 * t * k) & (N_EXT - 1)]));
            values[c * 64 + j] = acc;
        }
    }
    return values;
}

bool csr_ok(const uint32_t *start, size_t nrows, const uint32_t *order, size_t n) {
    if (start[0] != 0 || start[nrows] != n) return false;
    for (size_t t = 0; t < nrows; t++)
        if (start[t] > start[t + 1]) return false;
    for (size_t i = 0; i < n; i++)
        if (order[i] >= n) return false;
    return true;
}

}  // namespace

extern "C" {

static_assert(sizeof(Fr) == 32, "the limbs the tests pass");

// data [n_elems][8], in place: the count << logn elements of the transforms, then the guard
int ps_fr_ntt(uint32_t *data, size_t n_elems, const uint32_t *roots, size_t count, int logn, int dif, int inverse, int scale,
              int *rc) {
    if (!n_elems || n_elems > PS_MAX_ELEMS || logn < 0 || logn > 16 || count > PS_MAX_ELEMS || (count << logn) > n_elems)
        return DS_BAD_ARG;
    const Tables tb(roots);
    std::vector<Fr> v = fr_in(data, n_elems);
    std::vector<Arg> args = {{v.data(), v.data(), n_elems * 32, nullptr}};
    const size_t at = tb.push(args);
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        *rc = stage_ctx(ctx, st, args, at);
        if (*rc == 0) *rc = fr_ntt_batch(&ctx, (Fr *)args[0].dev, count, logn, dif != 0, inverse != 0, scale != 0);
    });
    if (run) return run;
    fr_out(data, v);
    return 0;
}

// out [out_elems][8] and bad [n_bad] go up as the caller filled them; in [total][32]; with_bad = 0: d_bad is null
int ps_bytes_to_fr(uint32_t *out, size_t out_elems, uint32_t *bad, size_t n_bad, const uint8_t *in, size_t total,
                   uint32_t elems_per_unit, int with_bad, int *rc) {
    if (!total || out_elems > PS_MAX_ELEMS || total > out_elems || !elems_per_unit || !n_bad ||
        (total + elems_per_unit - 1) / elems_per_unit > n_bad)
        return DS_BAD_ARG;
    std::vector<Fr> v = fr_in(out, out_elems);
    std::vector<Arg> args = {{v.data(), v.data(), out_elems * 32, nullptr}, {bad, bad, n_bad * 4, nullptr}, {in, nullptr, total * 32, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = bytes_to_fr_batch(&ctx, (Fr *)args[0].dev, with_bad ? (uint32_t *)args[1].dev : nullptr, (const uint8_t *)args[2].dev,
                                total, elems_per_unit);
    });
    if (run) return run;
    fr_out(out, v);
    return 0;
}

// out [out_bytes] goes up as the caller filled it; in [total][8]
int ps_fr_to_bytes(uint8_t *out, size_t out_bytes, const uint32_t *in, size_t total, int *rc) {
    if (!total || total > PS_MAX_ELEMS || out_bytes < total * 32) return DS_BAD_ARG;
    const std::vector<Fr> v = fr_in(in, total);
    std::vector<Arg> args = {{out, out, out_bytes, nullptr}, {v.data(), nullptr, total * 32, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = fr_to_bytes_batch(&ctx, (uint8_t *)args[0].dev, (const Fr *)args[1].dev, total);
    });
}

// dst [dst_elems][8] goes up as the caller filled it; src [count * n_src][8]
int ps_zero_extend(uint32_t *dst, size_t dst_elems, const uint32_t *src, size_t count, uint32_t n_src, uint32_t n_dst, int *rc) {
    if (!count || !n_src || n_src > n_dst || dst_elems > PS_MAX_ELEMS || count * n_dst > dst_elems) return DS_BAD_ARG;
    std::vector<Fr> d = fr_in(dst, dst_elems);
    const std::vector<Fr> s = fr_in(src, count * n_src);
    std::vector<Arg> args = {{d.data(), d.data(), dst_elems * 32, nullptr}, {s.data(), nullptr, s.size() * 32, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = zero_extend_batch(&ctx, (Fr *)args[0].dev, (const Fr *)args[1].dev, count, n_src, n_dst);
    });
    if (run) return run;
    fr_out(dst, d);
    return 0;
}

// y [n_out][8] and bad [n_out] go up as the caller filled them (n_out > n: the guard); blobs [K][131072], K <= 8;
// item i evaluates blob item_blob[i] at z[i].  The n blobs the stage reads are copies made on the device.
int ps_eval_blob_bytes(uint32_t *y, uint32_t *bad, size_t n_out, const uint8_t *blobs, size_t K, const uint32_t *item_blob,
                       const uint32_t *z, size_t n, const uint32_t *roots, int *rc) {
    if (!n || n > 4096 || n_out < n || n_out > 8192 || !K || K > 8) return DS_BAD_ARG;
    for (size_t i = 0; i < n; i++)
        if (item_blob[i] >= K) return DS_BAD_ARG;
    const Tables tb(roots);
    std::vector<Fr> yv = fr_in(y, n_out);
    const std::vector<Fr> zv = fr_in(z, n);
    std::vector<Arg> args = {{yv.data(), yv.data(), n_out * 32, nullptr},
                             {bad, bad, n_out * 4, nullptr},
                             {blobs, nullptr, K * BLOB_BYTES, nullptr},
                             {zv.data(), nullptr, n * 32, nullptr},
                             {nullptr, nullptr, n * BLOB_BYTES, nullptr}};
    const size_t at = tb.push(args);
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        *rc = stage_ctx(ctx, st, args, at);
        uint8_t *all = (uint8_t *)args[4].dev;
        for (size_t i = 0; i < n && *rc == 0; i++)
            if (hipMemcpyAsync(all + i * BLOB_BYTES, (const uint8_t *)args[2].dev + item_blob[i] * BLOB_BYTES, BLOB_BYTES,
                               hipMemcpyDeviceToDevice, st) != hipSuccess)
                *rc = DS_BAD_ARG;
        if (*rc == 0) *rc = eval_blob_bytes_batch_device(&ctx, (Fr *)args[0].dev, (uint32_t *)args[1].dev, all, (const Fr *)args[3].dev, n);
    });
    if (run) return run;
    fr_out(y, yv);
    return 0;
}

// y [n + 1][8], q [n + 1][4096][8] (canonical, as the stage writes them) and hit [n + 1] go up as the caller filled
// them; poly [n][4096][8]
int ps_eval_quotient(uint32_t *y, uint32_t *q, int32_t *hit, const uint32_t *poly, const uint32_t *z, size_t n,
                     const uint32_t *roots, int *rc) {
    if (!n || n > 64) return DS_BAD_ARG;
    const Tables tb(roots);
    std::vector<Fr> yv = fr_in(y, n + 1);
    const std::vector<Fr> pv = fr_in(poly, n * N_BLOB), zv = fr_in(z, n);
    std::vector<Arg> args = {{yv.data(), yv.data(), (n + 1) * 32, nullptr},
                             {q, q, (n + 1) * BLOB_BYTES, nullptr},
                             {hit, hit, (n + 1) * 4, nullptr},
                             {pv.data(), nullptr, pv.size() * 32, nullptr},
                             {zv.data(), nullptr, n * 32, nullptr}};
    const size_t at = tb.push(args);
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        *rc = stage_ctx(ctx, st, args, at);
        if (*rc == 0)
            *rc = eval_quotient_batch_device(&ctx, (Fr *)args[0].dev, (uint32_t *)args[1].dev, (int *)args[2].dev, (const Fr *)args[3].dev,
                                             (const Fr *)args[4].dev, n);
    });
    if (run) return run;
    fr_out(y, yv);
    return 0;
}

// a [n_elems][8] in place, b [n_elems][8]: the stage is told about the first n of them
int ps_fr_div_inplace(uint32_t *a, const uint32_t *b, size_t n_elems, size_t n, int *rc) {
    if (!n || n > n_elems || n_elems > PS_MAX_ELEMS) return DS_BAD_ARG;
    std::vector<Fr> av = fr_in(a, n_elems);
    const std::vector<Fr> bv = fr_in(b, n_elems);
    std::vector<Arg> args = {{av.data(), av.data(), n_elems * 32, nullptr}, {bv.data(), nullptr, n_elems * 32, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = fr_div_inplace_device(&ctx, (Fr *)args[0].dev, (const Fr *)args[1].dev, n);
    });
    if (run) return run;
    fr_out(a, av);
    return 0;
}

// a [n_elems][8] in place; b [period][8]
int ps_fr_mul_inplace(uint32_t *a, size_t n_elems, const uint32_t *b, size_t n, size_t period, int *rc) {
    if (!n || n > n_elems || n_elems > PS_MAX_ELEMS || !period || period > PS_MAX_ELEMS) return DS_BAD_ARG;
    std::vector<Fr> av = fr_in(a, n_elems);
    const std::vector<Fr> bv = fr_in(b, period);
    std::vector<Arg> args = {{av.data(), av.data(), n_elems * 32, nullptr}, {bv.data(), nullptr, period * 32, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = fr_mul_inplace_device(&ctx, (Fr *)args[0].dev, (const Fr *)args[1].dev, n, period);
    });
    if (run) return run;
    fr_out(a, av);
    return 0;
}

// z_domain, z_coset_inv [nsets + 1][128][8] go up as the caller filled them; masks [nsets][4]
int ps_recover_set_factors(uint32_t *z_domain, uint32_t *z_coset_inv, const uint32_t *masks, size_t nsets, const uint32_t *roots,
                           int *rc) {
    if (!nsets || nsets > 64) return DS_BAD_ARG;
    const Tables tb(roots);
    const size_t ne = (nsets + 1) * 128;
    std::vector<Fr> zd = fr_in(z_domain, ne), zi = fr_in(z_coset_inv, ne);
    std::vector<uint32_t> miss, miss_start = {0};   // the stage takes the sets as the plan hands them over
    for (size_t s = 0; s < nsets; s++) {
        coset_recover_missing(miss, masks + 4 * s, CELL_LOG);
        miss_start.push_back((uint32_t)miss.size());
    }
    miss.push_back(0);   // no empty upload where every set is full; no set owns this entry
    std::vector<Arg> args = {{zd.data(), zd.data(), ne * 32, nullptr}, {zi.data(), zi.data(), ne * 32, nullptr},
                             {miss.data(), nullptr, miss.size() * 4, nullptr}, {miss_start.data(), nullptr, miss_start.size() * 4, nullptr}};
    const size_t at = tb.push(args);
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        *rc = stage_ctx(ctx, st, args, at);
        if (*rc == 0)
            *rc = coset_recover_factors_enqueue(&ctx, (Fr *)args[0].dev, (Fr *)args[1].dev, (const uint32_t *)args[2].dev,
                                                (const uint32_t *)args[3].dev, nsets, CELL_LOG, coset_recover_parts(nsets, CELL_LOG));
    });
    if (run) return run;
    fr_out(z_domain, zd);
    fr_out(z_coset_inv, zi);
    return 0;
}

// a [nrows + 1][8192][8] in place; f [nsets][128][8]; row_set [nrows]
int ps_fr_mul_cell_factor(uint32_t *a, const uint32_t *f, size_t nsets, const uint32_t *row_set, size_t nrows, int *rc) {
    if (!nrows || nrows > 16 || !nsets || nsets > 64) return DS_BAD_ARG;
    for (size_t i = 0; i < nrows; i++)
        if (row_set[i] >= nsets) return DS_BAD_ARG;
    std::vector<Fr> av = fr_in(a, (nrows + 1) * N_EXT);
    const std::vector<Fr> fv = fr_in(f, nsets * 128);
    std::vector<Arg> args = {{av.data(), av.data(), av.size() * 32, nullptr}, {fv.data(), nullptr, fv.size() * 32, nullptr}, {row_set, nullptr, nrows * 4, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = fr_mul_coset_factor_enqueue(&ctx, (Fr *)args[0].dev, (const Fr *)args[1].dev, (const uint32_t *)args[2].dev, nrows, CELL_LOG);
    });
    if (run) return run;
    fr_out(a, av);
    return 0;
}

// image [num_rows + 1][128][2048] goes up as the caller filled it; cells [num_rows][num_cells][2048]; idx [num_cells]
int ps_scatter_cells(uint8_t *image, const uint8_t *cells, const uint32_t *idx, uint32_t num_cells, size_t num_rows, int *rc) {
    if (!num_cells || num_cells > 128 || !num_rows || num_rows > 16) return DS_BAD_ARG;
    for (uint32_t j = 0; j < num_cells; j++)
        if (idx[j] >= 128) return DS_BAD_ARG;
    std::vector<Arg> args = {{image, image, (num_rows + 1) * 128 * CELL_BYTES, nullptr},
                             {cells, nullptr, num_rows * num_cells * CELL_BYTES, nullptr},
                             {idx, nullptr, (size_t)num_cells * 4, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = scatter_cells_device(&ctx, (uint8_t *)args[0].dev, (const uint8_t *)args[1].dev, (const uint32_t *)args[2].dev, num_cells, num_rows);
    });
}

// image [image_rows + 1][128][2048] goes up as the caller filled it; cells [ncells][2048]; cell_dst [ncells] < image_rows * 128
int ps_scatter_cells_rows(uint8_t *image, size_t image_rows, const uint8_t *cells, const uint32_t *cell_dst, size_t ncells, int *rc) {
    if (!image_rows || image_rows > 16 || !ncells || ncells > 16 * 128) return DS_BAD_ARG;
    for (size_t i = 0; i < ncells; i++)
        if (cell_dst[i] >= image_rows * 128) return DS_BAD_ARG;
    std::vector<Arg> args = {{image, image, (image_rows + 1) * 128 * CELL_BYTES, nullptr},
                             {cells, nullptr, ncells * CELL_BYTES, nullptr},
                             {cell_dst, nullptr, ncells * 4, nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = scatter_cosets_rows_enqueue(&ctx, (uint8_t *)args[0].dev, (const uint8_t *)args[1].dev, (const uint32_t *)args[2].dev, ncells, CELL_LOG);
    });
}

// rows [nrows + 1][64][8] go up as the caller filled them; cell_fr [n][64][8]; rp [n][8]; row_start [nrows + 1]; order [n].
// grouped = 0: the aggregation of a single cell batch, coset_aggregate_device at cosets of 64 (nrows must be 128: its
// columns), else that of a chunk of groups, coset_group_aggregate_device at cosets of 64
int ps_cell_aggregate(uint32_t *rows, const uint32_t *cell_fr, const uint32_t *rp, const uint32_t *row_start, const uint32_t *order,
                      size_t n, size_t nrows, int grouped, int *rc) {
    if (!n || n * 64 > PS_MAX_ELEMS || !nrows || nrows > 4096 || (!grouped && nrows != 128)) return DS_BAD_ARG;
    if (!csr_ok(row_start, nrows, order, n)) return DS_BAD_ARG;
    std::vector<Fr> out = fr_in(rows, (nrows + 1) * 64);
    const std::vector<Fr> cv = fr_in(cell_fr, n * 64), rv = fr_in(rp, n);
    std::vector<Arg> args = {{out.data(), out.data(), out.size() * 32, nullptr},
                             {cv.data(), nullptr, cv.size() * 32, nullptr},
                             {rv.data(), nullptr, n * 32, nullptr},
                             {row_start, nullptr, (nrows + 1) * 4, nullptr},
                             {order, nullptr, n * 4, nullptr}};
    const int run = run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        if (grouped)
            *rc = coset_group_aggregate_device(&ctx, (Fr *)args[0].dev, (const Fr *)args[1].dev, (const Fr *)args[2].dev,
                                               (const uint32_t *)args[3].dev, (const uint32_t *)args[4].dev, n, nrows, CELL_LOG);
        else
            *rc = coset_aggregate_device(&ctx, (Fr *)args[0].dev, (const Fr *)args[1].dev, (const Fr *)args[2].dev,
                                         (const uint32_t *)args[3].dev, (const uint32_t *)args[4].dev, n, CELL_LOG);
    });
    if (run) return run;
    fr_out(rows, out);
    return 0;
}

// interp [128][8] (canonical, as the stage writes them: 64 values and a guard of 64) goes up as the caller filled it;
// cols [128][64][8]: the coefficients of each column's interpolation polynomial.  The stage of a single cell batch,
// coset_interp_device at cosets of 64, takes a column's VALUES (bit-reversed order) and makes the coefficients itself,
// so the shim evaluates each column first, on the host (values_of_coeffs64).
// (The stage on values, with its coefficients and partial rows read back: coset_verify_shim.hip.)
int ps_interp_sum(uint32_t *interp, const uint32_t *cols, const uint32_t *roots, int *rc) {
    const Tables tb(roots);
    const std::vector<Fr> values = values_of_coeffs64(tb, fr_in(cols, 128 * 64));
    std::vector<Arg> args = {{interp, interp, 128 * 32, nullptr},
                             {values.data(), nullptr, values.size() * 32, nullptr},
                             {nullptr, nullptr, (size_t)COSET_INTERP_BLOCKS * 64 * sizeof(Fr), nullptr}};
    const size_t at = tb.push(args);
    return run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        *rc = stage_ctx(ctx, st, args, at);
        if (*rc == 0) *rc = coset_interp_device(&ctx, (uint32_t *)args[0].dev, (Fr *)args[2].dev, (Fr *)args[1].dev, CELL_LOG);
    });
}

// sc [total][8] (canonical) goes up as the caller filled it; rows [nrows][64][8]: the coefficients of each row's
// interpolation polynomial; grp_rows [G + 1]; row_col [nrows];
// gd [4 G + 1]: start [G + 1] | first term of A_g [G] | distinct commitments of g [G] | first term of B_g [G].
// The stages of a chunk of groups, coset_group_interp_device and coset_group_interp_sum_device at cosets of 64: the first
// takes a row's VALUES and makes the coefficients itself, so the shim evaluates each row first, as ps_interp_sum does.
// (The stages on values, each with its whole buffer read back: coset_groups_shim.hip.)
int ps_group_interp_sum(uint32_t *sc, size_t total, const uint32_t *rows, size_t nrows, const uint32_t *grp_rows,
                        const uint32_t *row_col, const uint32_t *gd, size_t G, const uint32_t *roots, int *rc) {
    if (!G || G > 64 || !nrows || nrows > 4096 || !total || total > PS_MAX_ELEMS) return DS_BAD_ARG;
    if (grp_rows[0] != 0 || grp_rows[G] != nrows) return DS_BAD_ARG;
    for (size_t g = 0; g < G; g++) {
        if (grp_rows[g] > grp_rows[g + 1] || gd[g] > gd[g + 1]) return DS_BAD_ARG;
        const size_t cells = gd[g + 1] - gd[g];
        if (cells && (size_t)gd[G + 1 + g] + gd[2 * G + 1 + g] + cells + 64 > total) return DS_BAD_ARG;
    }
    for (size_t t = 0; t < nrows; t++)
        if (row_col[t] >= 128) return DS_BAD_ARG;
    const Tables tb(roots);
    const std::vector<Fr> rv = fr_in(rows, nrows * 64), values = values_of_coeffs64(tb, rv);
    std::vector<Arg> args = {{sc, sc, total * 32, nullptr},
                             {values.data(), nullptr, values.size() * 32, nullptr},
                             {grp_rows, nullptr, (G + 1) * 4, nullptr},
                             {row_col, nullptr, nrows * 4, nullptr},
                             {gd, nullptr, (4 * G + 1) * 4, nullptr}};
    const size_t at = tb.push(args);
    return run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        *rc = stage_ctx(ctx, st, args, at);
        if (*rc == 0) *rc = coset_group_interp_device(&ctx, (Fr *)args[1].dev, (const uint32_t *)args[3].dev, nrows, CELL_LOG);
        if (*rc == 0)
            *rc = coset_group_interp_sum_device(&ctx, (uint32_t *)args[0].dev, (const Fr *)args[1].dev, (const uint32_t *)args[2].dev,
                                                (const uint32_t *)args[4].dev, nrows, G, CELL_LOG);
    });
}

}  // extern "C"
