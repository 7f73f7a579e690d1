// Index maps of ckzg_hip_verify_cell_kzg_proof_batch_groups: everything the segmented kernels of verify.hip need to
// know about which cell belongs to which group, column and commitment, built on the host while the transcripts are
// being hashed.  Plain C++ (no HIP): host_shim.cpp replays the same maps on the CPU (tests/test_cell_groups_cpu.py).
//
// A chunk is G groups over N cells; group g is the slice [start[g], start[g + 1]).  Three kinds of segment:
//   pairs   the distinct (group, commitment) pairs, per group in order of first appearance -- the order in which the
//           reference deduplicates that slice's commitments (eip7594.c:345-376), so a pair's index inside its group is
//           the commitment index the group's transcript hashes;
//   rows    the distinct (group, column) pairs: one aggregated column each (eip7594.c:661-683), at most N of them;
//   jobs    two linear combinations per group, in the layout of group_jobs.hpp:
//                     A_g = [its commitments | its proofs | the 64 setup points of the interpolation commitment]
//                     B_g = [its proofs]
//           A_g's scalars are the weights, r^i h_k^64 and the negated interpolation coefficients, B_g's are r^i.
// Points are named by their index in the chunk's pool [N proofs | the chunk's distinct commitments | 64 setup points].
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "group_jobs.hpp"

namespace ckzg {

struct CellGroupsPlan : GroupJobs {
    size_t N = 0, G = 0, P = 0, R = 0;              // cells, groups, pairs, rows
    std::vector<uint32_t> cell_grp, cell_col;       // [N] group and column (< 128) of each cell
    std::vector<uint64_t> cell_pair;                // [N] index of the cell's commitment inside its group (the transcript's)
    std::vector<uint32_t> pair_off;                 // [G + 1] first pair of each group
    std::vector<uint32_t> pair_commit;              // [P] chunk-wide commitment id of each pair
    std::vector<uint32_t> pair_start, pair_members; // [P + 1], [N] cells of each pair
    std::vector<uint32_t> pair_term;                // [P] term (index into the jobs' layout) that carries the pair's weight
    std::vector<uint32_t> row_start, row_order;     // [R + 1], [N] cells of each row
    std::vector<uint32_t> row_col;                  // [R] column of each row
    std::vector<uint32_t> grp_rows;                 // [G + 1] first row of each group
    // [4 G + 1]: start[G + 1] | first term of A_g [G] | distinct commitments of g [G] | first term of B_g [G]
    std::vector<uint32_t> gd;
};

// start: G + 1 entries from 0 to N; cell_commit[i] < num_commits: the chunk-wide id of cell i's commitment;
// cell_indices[i] is taken modulo 128 (a group with an index out of range is invalid before it gets here and its
// result is never read).  Jobs use the four-lane ladders while all of them together stay within quad_max_terms.
inline void build_cell_groups_plan(CellGroupsPlan &p, const uint64_t *start, size_t G, const uint32_t *cell_commit,
                                   size_t num_commits, const uint64_t *cell_indices, size_t quad_max_terms) {
    const size_t N = (size_t)start[G];
    p.N = N;
    p.G = G;
    p.cell_grp.resize(N);
    p.cell_col.resize(N);
    p.cell_pair.resize(N);
    p.pair_off.assign(G + 1, 0);
    p.grp_rows.assign(G + 1, 0);
    p.pair_commit.clear();
    p.row_col.clear();
    std::vector<uint32_t> cell_row(N), cell_pair_abs(N);
    // stamps: which group last saw this commitment / column, and the pair / row it opened for it
    std::vector<uint32_t> seen_c(num_commits, 0xffffffffu), slot_c(num_commits, 0);
    uint32_t seen_col[128], slot_col[128];
    for (int c = 0; c < 128; c++) seen_col[c] = 0xffffffffu;
    for (size_t g = 0; g < G; g++) {
        p.pair_off[g] = (uint32_t)p.pair_commit.size();
        p.grp_rows[g] = (uint32_t)p.row_col.size();
        for (size_t i = (size_t)start[g]; i < (size_t)start[g + 1]; i++) {
            const uint32_t cm = cell_commit[i], col = (uint32_t)(cell_indices[i] & 127u);
            p.cell_grp[i] = (uint32_t)g;
            p.cell_col[i] = col;
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
            cell_pair_abs[i] = slot_c[cm];
            p.cell_pair[i] = slot_c[cm] - p.pair_off[g];
            cell_row[i] = slot_col[col];
        }
    }
    const size_t P = p.pair_commit.size(), R = p.row_col.size();
    p.P = P;
    p.R = R;
    p.pair_off[G] = (uint32_t)P;
    p.grp_rows[G] = (uint32_t)R;
    // cells of each pair and of each row: counting sorts
    auto csr = [N](std::vector<uint32_t> &first, std::vector<uint32_t> &list, const std::vector<uint32_t> &key, size_t nkeys) {
        first.assign(nkeys + 1, 0);
        list.resize(N);
        for (size_t i = 0; i < N; i++) first[key[i] + 1]++;
        for (size_t k = 0; k < nkeys; k++) first[k + 1] += first[k];
        std::vector<uint32_t> fill(first.begin(), first.begin() + nkeys);
        for (size_t i = 0; i < N; i++) list[fill[key[i]]++] = (uint32_t)i;
    };
    csr(p.pair_start, p.pair_members, cell_pair_abs, P);
    csr(p.row_start, p.row_order, cell_row, R);
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
            return !n ? 0 : b ? n : ncs[g] + n + 64;
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
                for (uint32_t k = 0; k < 64; k++) out.put(pool_setup + k);
            }
        });
}

}  // namespace ckzg
