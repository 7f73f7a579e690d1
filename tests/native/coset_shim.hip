// coset_shim.hip -- the column sum of the coset openings (g1_fft.hip: coset_colsum_enqueue, k_coset_colsum) behind a C
// ABI (tests/test_gpu_coset_stages.py).  ckzg_hip_compute_coset_kzg_proofs_batch reaches that stage with the products
// of honest blobs, which never meet an equal or an opposite operand; here the points are the caller's, so every
// partial sum is a known multiple of the generator.
//
// Linked WITH THE PRODUCT'S OBJECT FILES (Makefile: libcoset_shim.so), so the kernel is the product's binary code; the
// shim launches no kernel of its own.  The stage needs the stream of its DeviceCtx and nothing else.  Test aid only;
// its export is cos_* and is not part of libckzg_hip.so.  Calling convention: dev_shim_common.hpp.
#include "dev_shim_common.hpp"
#include "device.hpp"

using namespace ckzg;
using namespace ckzg::dev;

extern "C" {

static_assert(sizeof(G1XYZZ) == 192, "the strings the tests pass");

// u [rows][8192][192] goes up as the caller filled it and comes back whole: u[b][t] for t < 8192 >> e is the sum of
// the 2^e columns, what lies behind it is whatever the passes left there
int cos_colsum(uint8_t *u, size_t rows, int e, int *rc) {
    if (!rows || rows > 4 || e < 0 || e > 6) return DS_BAD_ARG;
    std::vector<Arg> args = {{u, u, rows * 8192 * sizeof(G1XYZZ), nullptr}};
    return run_bounded(args, [&](hipStream_t st) {
        DeviceCtx ctx;
        ctx.stream = st;
        *rc = coset_colsum_enqueue(&ctx, (G1XYZZ *)args[0].dev, e, rows);
    });
}

}  // extern "C"
