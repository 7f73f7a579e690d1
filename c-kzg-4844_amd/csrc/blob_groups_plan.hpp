// Index maps of ckzg_hip_verify_blob_kzg_proof_batch_groups: which blob belongs to which group and where the terms of
// every group's two sums lie, built on the host while the blobs cross PCIe.  Plain C++ (no HIP): host_shim.cpp replays
// the kernels over the same maps on the CPU (tests/test_blob_groups_cpu.py).
//
// A chunk is G groups over N blobs; group g is the slice [start[g], start[g + 1]) = [a, b).  Two linear combinations
// per group (eip4844.c:697-758 written as two sums), in the layout of group_jobs.hpp:
//     A_g = [C_a .. C_{b-1} | proof_a .. proof_{b-1} | G]      B_g = [proof_a .. proof_{b-1}]
// A_g's scalars are r_g^(i-a) on the commitments, r_g^(i-a) z_i on the proofs and -sum_i r_g^(i-a) y_i on the
// generator; B_g's are r_g^(i-a).  The group is valid iff e(A_g, [1]_2) e(-B_g, [s]_2) == 1.
// Points are named by their index in the chunk's pool [N commitments | N proofs | the G1 generator].
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "group_jobs.hpp"

namespace ckzg {

struct BlobGroupsPlan : GroupJobs {
    size_t N = 0, G = 0;                  // blobs, groups
    std::vector<uint32_t> blob_grp;       // [N] group of each blob
    std::vector<uint32_t> gd;             // [3 G + 1]: start[G + 1] | first term of A_g [G] | first term of B_g [G]
};

// start: G + 1 entries from 0 to N.  Jobs use the four-lane ladders while all of them together stay within
// quad_max_terms.
inline void build_blob_groups_plan(BlobGroupsPlan &p, const uint64_t *start, size_t G, size_t quad_max_terms) {
    const size_t N = (size_t)start[G];
    p.N = N;
    p.G = G;
    p.blob_grp.resize(N);
    p.gd.assign(3 * G + 1, 0);
    uint32_t *gstart = p.gd.data(), *term_a = gstart + G + 1, *term_b = term_a + G;
    for (size_t g = 0; g <= G; g++) gstart[g] = (uint32_t)start[g];
    for (size_t g = 0; g < G; g++) {
        for (uint32_t i = gstart[g]; i < gstart[g + 1]; i++) p.blob_grp[i] = (uint32_t)g;
    }
    const uint32_t pool_proof = (uint32_t)N, pool_gen = (uint32_t)(2 * N);
    lay_out_group_jobs(
        p, G, quad_max_terms, term_a, term_b,
        [&](size_t g, bool b) -> size_t {
            const size_t n = gstart[g + 1] - gstart[g];
            return !n ? 0 : b ? n : 2 * n + 1;
        },
        [&](size_t g, bool b, GroupJobTerms &out) {
            const uint32_t a = gstart[g], n = gstart[g + 1] - a;
            if (!n) return;
            if (!b) {
                for (uint32_t i = 0; i < n; i++) out.put(a + i);
            }
            for (uint32_t i = 0; i < n; i++) out.put(pool_proof + a + i);
            if (!b) out.put(pool_gen);
        });
}

}  // namespace ckzg
