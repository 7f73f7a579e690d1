// Index maps of ckzg_hip_verify_blob_kzg_proof_batch_groups: which blob belongs to which group and where the terms of
// every group's two sums lie, built on the host while the blobs cross PCIe.  Plain C++ (no HIP): host_shim.cpp replays
// the kernels over the same maps on the CPU (tests/test_blob_groups_cpu.py).
//
// A chunk is G groups over N blobs; group g is the slice [start[g], start[g + 1]) = [a, b).  Two linear combinations
// per group (eip4844.c:697-758 written as two sums), laid out job after job and padded to a whole partial of the ladder
// kernels, as in cell_groups_plan.hpp:
//     A_g = [C_a .. C_{b-1} | proof_a .. proof_{b-1} | G]      B_g = [proof_a .. proof_{b-1}]
// A_g's scalars are r_g^(i-a) on the commitments, r_g^(i-a) z_i on the proofs and -sum_i r_g^(i-a) y_i on the
// generator; B_g's are r_g^(i-a).  The group is valid iff e(A_g, [1]_2) e(-B_g, [s]_2) == 1.  An empty group has two
// empty jobs (the empty sum: infinity).
// Points are named by their index in the chunk's pool [N commitments | N proofs | the G1 generator].
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cell_groups_plan.hpp"   // CELL_GROUPS_NO_POINT: a padding term

namespace ckzg {

struct BlobGroupsPlan {
    size_t N = 0, G = 0, total = 0;       // blobs, groups, terms of all jobs (padded)
    bool quad = false;                    // jobs padded to 8 terms (four-lane ladders) or to 32
    std::vector<uint32_t> blob_grp;       // [N] group of each blob
    std::vector<uint32_t> gd;             // [3 G + 1]: start[G + 1] | first term of A_g [G] | first term of B_g [G]
    std::vector<uint32_t> term_src;       // [total] pool index of each term's point, or CELL_GROUPS_NO_POINT
    std::vector<uint32_t> part_off;       // [2 G + 1] first partial of each job (A_0, B_0, A_1, ...)
    size_t per() const { return quad ? 8 : 32; }
};

// start: G + 1 entries from 0 to N.  Jobs use the four-lane ladders while all of them together stay within
// quad_max_terms.
inline void build_blob_groups_plan(BlobGroupsPlan &p, const uint64_t *start, size_t G, size_t quad_max_terms) {
    const size_t N = (size_t)start[G];
    p.N = N;
    p.G = G;
    p.blob_grp.resize(N);
    auto padded = [](size_t n, size_t per) { return (n + per - 1) / per * per; };
    size_t total8 = 0;
    for (size_t g = 0; g < G; g++) {
        const size_t n = (size_t)(start[g + 1] - start[g]);
        for (size_t i = (size_t)start[g]; i < (size_t)start[g + 1]; i++) p.blob_grp[i] = (uint32_t)g;
        if (n) total8 += padded(2 * n + 1, 8) + padded(n, 8);
    }
    p.quad = total8 <= quad_max_terms;
    const size_t per = p.per();
    p.gd.assign(3 * G + 1, 0);
    p.part_off.assign(2 * G + 1, 0);
    p.term_src.clear();
    uint32_t *gstart = p.gd.data(), *term_a = gstart + G + 1, *term_b = term_a + G;
    const uint32_t pool_proof = (uint32_t)N, pool_gen = (uint32_t)(2 * N);
    for (size_t g = 0; g < G; g++) {
        const size_t a = (size_t)start[g], n = (size_t)(start[g + 1] - start[g]);
        gstart[g] = (uint32_t)a;
        term_a[g] = (uint32_t)p.term_src.size();
        p.part_off[2 * g] = (uint32_t)(p.term_src.size() / per);
        if (n) {
            for (size_t i = 0; i < n; i++) p.term_src.push_back((uint32_t)(a + i));
            for (size_t i = 0; i < n; i++) p.term_src.push_back(pool_proof + (uint32_t)(a + i));
            p.term_src.push_back(pool_gen);
            p.term_src.resize(padded(p.term_src.size(), per), CELL_GROUPS_NO_POINT);
        }
        term_b[g] = (uint32_t)p.term_src.size();
        p.part_off[2 * g + 1] = (uint32_t)(p.term_src.size() / per);
        if (n) {
            for (size_t i = 0; i < n; i++) p.term_src.push_back(pool_proof + (uint32_t)(a + i));
            p.term_src.resize(padded(p.term_src.size(), per), CELL_GROUPS_NO_POINT);
        }
    }
    gstart[G] = (uint32_t)N;
    p.total = p.term_src.size();
    p.part_off[2 * G] = (uint32_t)(p.total / per);
    // the ladder kernels take a multiple of 64 terms
    p.term_src.resize(padded(p.total, 64), CELL_GROUPS_NO_POINT);
    p.total = p.term_src.size();
}

}  // namespace ckzg
