// fk20_shim.hip -- the two length-128 G1 transforms of FK20 (fk20.hip: fk20_fft_stage_enqueue) behind a C ABI
// (tests/test_gpu_fk20_stages.py).  compute_cells_and_kzg_proofs and recover_cells_and_kzg_proofs reach that stage with
// the sums of honest blobs, which never meet an equal or an opposite operand; here the points are the caller's, so
// every output is a known multiple of the generator.
//
// What the stage computes on each of its n vectors u[0..127], with w = W128 (w^128 = 1):
//     out[k] = sum_{j < 64} w^(jk) * sum_{f < 128} w^(-fj) u[f]
// the inverse transform, its upper half dropped, the forward transform.  There is no factor 1/128: the product folds it
// into the scalars of the MSMs that make u.  `out` is in the order the stage leaves it, which is the natural order k
// (tests/test_gpu_fk20_stages.py confirms it: the expected points of the tones, which are not symmetric in k, are the
// oracle's multiples of the generator and are met at k, not at brp7(k)); k_compress applies the bit reversal of the
// proofs afterwards.  Which of the six forms runs is the decision of
// fk20_fft_plan.hpp for n; the shim reports it.
//
// Linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libfk20_shim.so), so every kernel is the product's binary code; the
// shim launches no kernel of its own.  The stage needs the stream of its DeviceCtx and d_roots, from which the product's
// own k_glv_roots makes the twiddle records on first use: the shim fills d_roots with the powers of the setup's root of
// unity as compute_roots_of_unity does (ckzg_api.hip).  No trusted setup.  Test aid only; its export is fks_* and is
// not part of libckzg_hip.so.  Calling convention: dev_shim_common.hpp.
#include <cstring>
#include "dev_shim_common.hpp"
#include "device.hpp"
#include "fk20_fft_plan.hpp"

using namespace ckzg;
using namespace ckzg::dev;

namespace {

constexpr size_t FKS_MAX_TRANSFORMS = 640;   // past the last hand-over (512 | 513) with room for a partial wave
constexpr size_t FKS_GUARD_POINTS = 128;     // one more vector than the stage is told about, behind u
constexpr size_t FKS_GUARD_BYTES = 4096;     // behind the stage's scratch, filled with FKS_GUARD_FILL
constexpr uint8_t FKS_GUARD_FILL = 0xa5;
constexpr int FKS_SCRATCH_OVERRUN = 9997;    // the stage wrote behind the scratch it asked for

}  // namespace

extern "C" {

static_assert(sizeof(G1XYZZ) == 192, "the strings the tests pass");

// u [n + 1][128][192] goes up as the caller filled it -- n vectors and a guard vector -- and comes back whole.  The
// stage's scratch has a guard of its own behind it, which the shim fills and checks (9997 if it was written).
// *form_out: the form the stage took.
int fks_transforms(uint8_t *u, size_t n, int *form_out, int *rc) {
    if (!n || n > FKS_MAX_TRANSFORMS) return DS_BAD_ARG;
    std::vector<Fr> roots(N_EXT + 1);
    Fr root;
    for (int i = 0; i < 8; i++) root.l[i] = FR_ROOT_8192_MONT[i];
    roots[0] = Fr::one();
    for (int i = 1; i <= N_EXT; i++) roots[i] = mul(roots[i - 1], root);
    const size_t sbytes = fk20_fft_scratch_bytes(n);
    std::vector<uint8_t> scratch(sbytes + FKS_GUARD_BYTES, 0);
    memset(scratch.data() + sbytes, FKS_GUARD_FILL, FKS_GUARD_BYTES);
    std::vector<Arg> args = {{u, u, (n * 128 + FKS_GUARD_POINTS) * sizeof(G1XYZZ), nullptr},
                             {scratch.data(), scratch.data(), scratch.size(), nullptr},
                             {roots.data(), nullptr, roots.size() * sizeof(Fr), nullptr}};
    DeviceCtx ctx;
    *form_out = fk20_fft_form_for(n);
    const int run = run_bounded(args, [&](hipStream_t st) {
        ctx.stream = st;
        ctx.d_roots = (Fr *)args[2].dev;
        *rc = fk20_fft_stage_enqueue(&ctx, (G1XYZZ *)args[0].dev, (uint8_t *)args[1].dev, n);
    });
    if (run == DS_DEADLINE) return run;   // nothing is freed under a running kernel
    if (ctx.d_roots_raw) (void)hipFree(ctx.d_roots_raw);
    if (run) return run;
    for (size_t i = 0; i < FKS_GUARD_BYTES; i++)
        if (scratch[sbytes + i] != FKS_GUARD_FILL) return FKS_SCRATCH_OVERRUN;
    return 0;
}

}  // extern "C"
