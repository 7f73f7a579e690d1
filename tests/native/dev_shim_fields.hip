// dev_shim_fields.hip -- the device forms of field_test_ops.hpp behind a C ABI: Mont<Fp> / Mont<Fr> on the 32-bit CIOS,
// Fr29 (the called product fr29_mul_regs among it), the safegcd inversions and the pairing tower of tower.hpp /
// pairing_dev.hpp with its out-of-line products, as the DEVICE compiler builds them.  Compiled ONCE, with the product's
// plain flags -- what pairing.o, verify.o and ntt.o are built with -- and linked into libdev_shim.so next to
// dev_shim.hip's two forms; its exports are ds_dev_*.  Test aid only (tests/test_gpu_fields.py); never part of
// libckzg_hip.so.
//
// The rules of dev_shim.hip hold: host pointers in, ONE kernel per call on a stream of its own, a polling 20 s
// deadline (dev_shim_common.hpp), bounded loops only.  Geometry: one thread per item in workgroups of `block` threads;
// lanes past n repeat the last item and store nothing, as k_point_lhs / k_pairing_check do, so that a wave is never
// partly idle inside the pairing.
#include "dev_shim_common.hpp"
#include "field_test_ops.hpp"

using namespace ckzg;

// s*: the distance in words between two items' operands (0: shared by all items)
__global__ __launch_bounds__(MAX_BLOCK) void ds_dev_k_field(int op, uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c,
                                                            const uint32_t *d, int so, int sa, int sb, int sc, int sd, int n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const bool live = i < (size_t)n;
    if (!live) i = (size_t)n - 1;
    uint32_t o[fieldtest::MAX_WORDS];
    for (int j = 0; j < fieldtest::MAX_WORDS; j++) o[j] = 0;
    if (!fieldtest::run(op, o, a + (size_t)sa * i, b + (size_t)sb * i, c + (size_t)sc * i, d + (size_t)sd * i)) return;
    if (live)
        for (int j = 0; j < so; j++) out[(size_t)so * i + j] = o[j];
}

extern "C" {

const char *ds_dev_field_ops() { return fieldtest::desc(); }

// n items; operand k of item i lies at k + width * i, a shared operand (line tables) at k: the widths are the list's
int ds_dev_field(int op, uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, int n, int block) {
    int w[6];
    if (!geometry_ok(n, block) || !fieldtest::widths(op, w)) return DS_BAD_ARG;
    if (w[0] <= 0 || w[0] > fieldtest::MAX_WORDS) return DS_BAD_ARG;
    const int sc = w[5] ? 0 : w[3], sd = w[5] ? 0 : w[4];
    auto bytes = [&](int width, int stride) { return (size_t)width * 4 * (stride ? (size_t)n : 1); };
    std::vector<Arg> args = {{nullptr, out, bytes(w[0], w[0])}, {w[1] ? a : nullptr, nullptr, bytes(w[1], w[1])},
                             {w[2] ? b : nullptr, nullptr, bytes(w[2], w[2])}, {w[3] ? c : nullptr, nullptr, bytes(w[3], sc)},
                             {w[4] ? d : nullptr, nullptr, bytes(w[4], sd)}};
    return run_bounded(args, [&](hipStream_t st) {
        hipLaunchKernelGGL(ds_dev_k_field, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, op, (uint32_t *)args[0].dev,
                           (const uint32_t *)args[1].dev, (const uint32_t *)args[2].dev, (const uint32_t *)args[3].dev,
                           (const uint32_t *)args[4].dev, w[0], w[1], w[2], sc, sd, n);
    });
}

}  // extern "C"
