// coset_verify_plan.hpp -- the index arithmetic and the launch decisions of ckzg_hip_verify_coset_kzg_proof_batch and,
// at e = 6, of verify_cell_kzg_proof_batch (coset_verify.hip), once, for the host and for the kernels (HD), and through libhost_shim.so
// for the CPU tests (tests/test_coset_verify_cpu.py; the model is tests/coset_verify_expect.py).
//
// Coset size l = 2^e, e <= COSET_MAX_LOG; m = 8192 >> e cosets.  With w = roots_of_unity[1] of the 8192-point domain,
// coset c is x_c times the l-th roots of unity, x_c = w^brp_{13-e}(c), and value j of an item sits at
// x_c * w_l^brp_e(j), w_l = w^(8192 / l): the order of brp_roots_of_unity[c l .. c l + l - 1].
#pragma once
#include <cstddef>
#include <cstdint>

#include "field.hpp"
#include "g1_fft_plan.hpp"

namespace ckzg {

constexpr uint32_t COSET_VERIFY_EXT = 8192;   // points of the extended domain = slots of the aggregate, whatever e is

HD uint32_t coset_verify_cosets(int e) { return COSET_VERIFY_EXT >> e; }

// brp_{13-e}(c): the exponent of x_c = w^brp_{13-e}(c); c < 8192 >> e
HD uint32_t coset_verify_brp(uint32_t c, int e) {
    uint32_t r = 0;
    for (int b = 0; b < 13 - e; b++) r |= ((c >> b) & 1u) << (12 - e - b);
    return r;
}
// index into roots_of_unity of x_c^l, the factor of the proof in the check
HD uint32_t coset_verify_shift_root(uint32_t c, int e) { return (coset_verify_brp(c, e) << e) & (COSET_VERIFY_EXT - 1u); }
// index into roots_of_unity of x_c^-k = w^((8192 - brp_{13-e}(c)) k), k < l
HD uint32_t coset_verify_unshift_root(uint32_t c, int e, uint32_t k) {
    return ((COSET_VERIFY_EXT - coset_verify_brp(c, e)) * k) & (COSET_VERIFY_EXT - 1u);
}
// slot of value j of coset c in the aggregate: m columns of l, back to back
HD uint32_t coset_verify_slot(uint32_t c, int e, uint32_t j) { return (c << e) + j; }

// The inverse transform of a column: input in bit-reversed order, output natural.  Stage s = 1 .. e has butterflies of
// span half = 2^(s-1); position pos of a column pairs with pos ^ half, and the upper input is multiplied by
// w_{2^s}^-(pos mod half), whose index into roots_of_unity is this:
HD uint32_t coset_verify_twiddle_root(uint32_t pos, int s) {
    const uint32_t half = 1u << (s - 1), t = pos & (half - 1u);
    return (COSET_VERIFY_EXT - t * (COSET_VERIFY_EXT >> s)) & (COSET_VERIFY_EXT - 1u);
}

// Aggregation: one lane per slot and part.  A column with many items is split over `parts` lanes per slot, each taking
// every parts-th item of the column's list, and the parts are folded in LDS.  parts is a power of two, grows while an
// average column would give a lane more than COSET_AGG_ITEMS_PER_LANE items, and stops at COSET_AGG_MAX_PARTS (1024
// threads, 32 KB of LDS).  The aggregation by groups (coset_groups_plan.hpp) takes the same numbers.
constexpr uint32_t COSET_AGG_ITEMS_PER_LANE = 4;
constexpr uint32_t COSET_AGG_MAX_PARTS = 16;
constexpr uint32_t COSET_AGG_SLOTS_PER_BLOCK = 64;
HD uint32_t coset_verify_agg_parts(uint64_t items, int e) {
    uint32_t parts = 1;
    while (parts < COSET_AGG_MAX_PARTS && (uint64_t)parts * coset_verify_cosets(e) * COSET_AGG_ITEMS_PER_LANE < items) parts <<= 1;
    return parts;
}

// Interpolation and fold: workgroups of COSET_INTERP_THREADS consecutive slots (whole columns: l <= 64 divides it).
// A workgroup transforms its columns in LDS, multiplies by x_c^-k / l and folds its columns onto l partial sums; a
// second launch adds the COSET_VERIFY_EXT / COSET_INTERP_THREADS partial rows.
constexpr uint32_t COSET_INTERP_THREADS = 256;
constexpr uint32_t COSET_INTERP_BLOCKS = COSET_VERIFY_EXT / COSET_INTERP_THREADS;

// The transcript of a batch: the reference's (eip7594.c:390-482) with the cell size a parameter.  "RCKZGCBATCH__V1_" |
// be64 4096 | be64 l | be64 distinct commitments | be64 items, the distinct commitments in order of first appearance,
// then per item be64 commitment index | be64 coset index | its l values (32 bytes each) | its proof.  The challenge is
// the digest reduced mod r.  At l = 64 this is the input of compute_verify_cell_kzg_proof_batch_challenge, byte for byte.
template <class Sha>
void coset_verify_digest(uint8_t digest[32], const uint8_t *commitments48, uint64_t num_commitments,
                         const uint64_t *commitment_indices, const uint64_t *coset_indices, const uint8_t *evals32,
                         const uint8_t *proofs48, uint64_t num_cosets, int e) {
    auto put64 = [](uint8_t *out, uint64_t v) {
        for (int i = 0; i < 8; i++) out[i] = (uint8_t)(v >> (56 - 8 * i));
    };
    const uint64_t l = (uint64_t)1 << e;
    Sha h;
    uint8_t head[48], idx[16];
    __builtin_memcpy(head, "RCKZGCBATCH__V1_", 16);
    put64(head + 16, 4096);
    put64(head + 24, l);
    put64(head + 32, num_commitments);
    put64(head + 40, num_cosets);
    h.update(head, 48);
    h.update(commitments48, 48 * num_commitments);
    for (uint64_t i = 0; i < num_cosets; i++) {
        put64(idx, commitment_indices[i]);
        put64(idx + 8, coset_indices[i]);
        h.update(idx, 16);
        h.update(evals32 + 32 * l * i, 32 * l);
        h.update(proofs48 + 48 * i, 48);
    }
    h.finish(digest);
}

// From this many items on, the transcript is hashed on the worker pool underneath copies and validation
constexpr uint64_t COSET_VERIFY_HASH_ON_POOL_FROM = 256;

// Several devices: no shard below this many items, whatever e is -- an item's cost is its proof's (decompression,
// subgroup test, two ladders or table sums); verify_cell_kzg_proof_batch is this check at e = 6
constexpr uint64_t COSET_VERIFY_MIN_SHARD = 2048;

}  // namespace ckzg
