// Index maps and launch decisions of the cell check by groups at coset size l = 2^e, e <= COSET_MAX_LOG
// (ckzg_hip_verify_coset_kzg_proof_batch_groups at its e; the cell and the blob-cell calls by groups at e = 6, where a
// coset is a cell and a coset index a column) -- everything the segmented kernels of coset_groups.hip need to know about
// which item belongs to which group, coset and commitment, built on the host while the transcripts are being hashed.
// Plain C++ (no HIP): host_shim.cpp replays the same maps on the CPU (tests/test_coset_groups_cpu.py,
// tests/test_cell_groups_cpu.py).  DESIGN.md sections 3b and 3i.2.
//
// A chunk is G groups over N items; group g is the slice [start[g], start[g + 1]).  Three kinds of segment:
//   pairs   the distinct (group, commitment) pairs, per group in order of first appearance -- the order in which
//           coset_verify_digest wants the slice's commitments (the reference's deduplication, eip7594.c:345-376), so a
//           pair's index inside its group is the commitment index the group's transcript hashes;
//   rows    the distinct (group, coset) pairs: one aggregated column of l values each, at most N of them, the rows of a
//           group back to back -- R l slots, over which the kernels map their lanes;
//   jobs    two linear combinations per group, in the layout of group_jobs.hpp:
//                     A_g = [its commitments | its proofs | the first l setup points]
//                     B_g = [its proofs]
//           A_g's scalars are the weights, r^i x_c^l and the negated interpolation coefficients, B_g's are r^i.
// Points are named by their index in the chunk's pool [N proofs | the chunk's distinct commitments | l setup points].
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "coset_verify_plan.hpp"
#include "group_jobs.hpp"

namespace ckzg {

struct CosetGroupsPlan : GroupJobs {
    int e = 0;
    size_t N = 0, G = 0, P = 0, R = 0;              // items, groups, pairs, rows
    std::vector<uint32_t> item_grp, item_col;       // [N] group and coset (< 8192 >> e) of each item
    std::vector<uint64_t> item_pair;                // [N] index of the item's commitment inside its group (the transcript's)
    std::vector<uint32_t> pair_off;                 // [G + 1] first pair of each group
    std::vector<uint32_t> pair_commit;              // [P] chunk-wide commitment id of each pair
    std::vector<uint32_t> pair_start, pair_members; // [P + 1], [N] items of each pair
    std::vector<uint32_t> pair_term;                // [P] term (index into the jobs' layout) that carries the pair's weight
    std::vector<uint32_t> row_start, row_order;     // [R + 1], [N] items of each row
    std::vector<uint32_t> row_col;                  // [R] coset of each row
    std::vector<uint32_t> grp_rows;                 // [G + 1] first row of each group
    // [4 G + 1]: start[G + 1] | first term of A_g [G] | distinct commitments of g [G] | first term of B_g [G]
    std::vector<uint32_t> gd;
};

// start: G + 1 entries from 0 to N; item_commit[i] < num_commits: the chunk-wide id of item i's commitment;
// coset_indices[i] is taken modulo m = 8192 >> e (a group with an index out of range is invalid before it gets here and
// its result is never read).  Jobs use the four-lane ladders while all of them together stay within quad_max_terms.
inline void build_coset_groups_plan(CosetGroupsPlan &p, const uint64_t *start, size_t G, const uint32_t *item_commit,
                                    size_t num_commits, const uint64_t *coset_indices, int e, size_t quad_max_terms) {
    const size_t N = (size_t)start[G], l = (size_t)1 << e;
    const uint32_t m = coset_verify_cosets(e);
    p.e = e;
    p.N = N;
    p.G = G;
    p.item_grp.resize(N);
    p.item_col.resize(N);
    p.item_pair.resize(N);
    p.pair_off.assign(G + 1, 0);
    p.grp_rows.assign(G + 1, 0);
    p.pair_commit.clear();
    p.row_col.clear();
    std::vector<uint32_t> item_row(N), item_pair_abs(N);
    // stamps: which group last saw this commitment / coset, and the pair / row it opened for it
    std::vector<uint32_t> seen_c(num_commits, 0xffffffffu), slot_c(num_commits, 0);
    std::vector<uint32_t> seen_col(m, 0xffffffffu), slot_col(m, 0);
    for (size_t g = 0; g < G; g++) {
        p.pair_off[g] = (uint32_t)p.pair_commit.size();
        p.grp_rows[g] = (uint32_t)p.row_col.size();
        for (size_t i = (size_t)start[g]; i < (size_t)start[g + 1]; i++) {
            const uint32_t cm = item_commit[i], col = (uint32_t)(coset_indices[i] & (m - 1u));
            p.item_grp[i] = (uint32_t)g;
            p.item_col[i] = col;
            if (seen_c[cm] != (uint32_t)g) {
                seen_c[cm] = (uint32_t)g;
                slot_c[cm] = (uint32_t)p.pair_commit.size();
                p.pair_commit.push_back(cm);
            }
            if (seen_col[col] != (uint32_t)g) {
                seen_col[col] = (uint32_t)g;
                slot_col[col] = (uint32_t)p.row_col.size();
                p.row_col.push_back(col);
            }
            item_pair_abs[i] = slot_c[cm];
            p.item_pair[i] = slot_c[cm] - p.pair_off[g];
            item_row[i] = slot_col[col];
        }
    }
    const size_t P = p.pair_commit.size(), R = p.row_col.size();
    p.P = P;
    p.R = R;
    p.pair_off[G] = (uint32_t)P;
    p.grp_rows[G] = (uint32_t)R;
    // items of each pair and of each row: counting sorts
    auto csr = [N](std::vector<uint32_t> &first, std::vector<uint32_t> &list, const std::vector<uint32_t> &key, size_t nkeys) {
        first.assign(nkeys + 1, 0);
        list.resize(N);
        for (size_t i = 0; i < N; i++) first[key[i] + 1]++;
        for (size_t k = 0; k < nkeys; k++) first[k + 1] += first[k];
        std::vector<uint32_t> fill(first.begin(), first.begin() + nkeys);
        for (size_t i = 0; i < N; i++) list[fill[key[i]]++] = (uint32_t)i;
    };
    csr(p.pair_start, p.pair_members, item_pair_abs, P);
    csr(p.row_start, p.row_order, item_row, R);
    // the jobs
    p.gd.assign(4 * G + 1, 0);
    p.pair_term.resize(P);
    uint32_t *gstart = p.gd.data(), *term_a = gstart + G + 1, *ncs = term_a + G, *term_b = ncs + G;
    for (size_t g = 0; g <= G; g++) gstart[g] = (uint32_t)start[g];
    for (size_t g = 0; g < G; g++) ncs[g] = p.pair_off[g + 1] - p.pair_off[g];
    const uint32_t pool_commit = (uint32_t)N, pool_setup = (uint32_t)(N + num_commits);
    lay_out_group_jobs(
        p, G, quad_max_terms, term_a, term_b,
        [&](size_t g, bool b) -> size_t {
            const size_t n = gstart[g + 1] - gstart[g];
            return !n ? 0 : b ? n : ncs[g] + n + l;
        },
        [&](size_t g, bool b, GroupJobTerms &out) {
            const uint32_t a = gstart[g], n = gstart[g + 1] - a;
            if (!n) return;
            if (!b) {
                for (uint32_t j = p.pair_off[g]; j < p.pair_off[g + 1]; j++) {
                    p.pair_term[j] = out.at();
                    out.put(pool_commit + p.pair_commit[j]);
                }
            }
            for (uint32_t i = 0; i < n; i++) out.put(a + i);
            if (!b) {
                for (uint32_t k = 0; k < (uint32_t)l; k++) out.put(pool_setup + k);
            }
        });
}

// ---- launch pickers of coset_groups.hip ----

// k_coset_group_aggregate: one lane per (row slot, part) over the R l slots, COSET_AGG_SLOTS_PER_BLOCK slots a workgroup.
// The parts rule is coset_verify_agg_parts' with the chunk's rows in the place of the m columns: a power of two that
// grows while an average row would give a lane more than COSET_AGG_ITEMS_PER_LANE items, at most COSET_AGG_MAX_PARTS
// (1024 threads, 32 KB of LDS).  The switch points are those of the single check, unmeasured for this call.
HD uint32_t coset_groups_agg_parts(uint64_t items, uint64_t rows) {
    uint32_t parts = 1;
    while (parts < COSET_AGG_MAX_PARTS && (uint64_t)parts * rows * COSET_AGG_ITEMS_PER_LANE < items) parts <<= 1;
    return parts;
}
HD uint64_t coset_groups_agg_blocks(uint64_t rows, int e) {
    return ((rows << e) + COSET_AGG_SLOTS_PER_BLOCK - 1) / COSET_AGG_SLOTS_PER_BLOCK;
}

// k_coset_group_interp: COSET_INTERP_THREADS consecutive row slots a workgroup -- whole rows, since l <= 64 divides it
HD uint64_t coset_groups_interp_blocks(uint64_t rows, int e) {
    return ((rows << e) + COSET_INTERP_THREADS - 1) / COSET_INTERP_THREADS;
}

// k_coset_group_interp_sum: one lane per (output, part) over the G l outputs, COSET_GROUPS_SUM_OUT_PER_BLOCK outputs a
// workgroup; part p of an output adds every parts-th row of its group from the p-th on, and the parts are folded in
// LDS.  parts is a power of two that grows while an average group would give a lane more than
// COSET_GROUPS_SUM_ROWS_PER_LANE rows, at most COSET_GROUPS_SUM_MAX_PARTS: a cell group has at most 128 rows, which
// four parts bring to 32 a lane, and this rule keeps that for the average group at every e.  Switch points set by this
// reasoning alone: unmeasured.
constexpr uint32_t COSET_GROUPS_SUM_OUT_PER_BLOCK = 64;
constexpr uint32_t COSET_GROUPS_SUM_ROWS_PER_LANE = 32;
constexpr uint32_t COSET_GROUPS_SUM_MAX_PARTS = 16;
HD uint32_t coset_groups_sum_parts(uint64_t rows, uint64_t groups) {
    uint32_t parts = 1;
    while (parts < COSET_GROUPS_SUM_MAX_PARTS && (uint64_t)parts * groups * COSET_GROUPS_SUM_ROWS_PER_LANE < rows) parts <<= 1;
    return parts;
}
HD uint64_t coset_groups_sum_blocks(uint64_t groups, int e) {
    return ((groups << e) + COSET_GROUPS_SUM_OUT_PER_BLOCK - 1) / COSET_GROUPS_SUM_OUT_PER_BLOCK;
}

}  // namespace ckzg
