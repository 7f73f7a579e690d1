// Index maps of ckzg_hip_verify_cell_kzg_proof_batch_groups: everything the segmented kernels of verify.hip need to
// know about which cell belongs to which group, column and commitment, built on the host while the transcripts are
// being hashed.  Plain C++ (no HIP): host_shim.cpp replays the same maps on the CPU (tests/test_cell_groups_cpu.py).
//
// A chunk is G groups over N cells; group g is the slice [start[g], start[g + 1]).  Three kinds of segment:
//   pairs   the distinct (group, commitment) pairs, per group in order of first appearance -- the order in which the
//           reference deduplicates that slice's commitments (eip7594.c:345-376), so a pair's index inside its group is
//           the commitment index the group's transcript hashes;
//   rows    the distinct (group, column) pairs: one aggregated column each (eip7594.c:661-683), at most N of them;
//   jobs    two linear combinations per group, laid out job after job and padded to a whole partial of the ladder
//           kernels:  A_g = [its commitments | its proofs | the 64 setup points of the interpolation commitment]
//                     B_g = [its proofs]
//           A_g's scalars are the weights, r^i h_k^64 and the negated interpolation coefficients, B_g's are r^i.
//           An empty group has two empty jobs (the empty sum: infinity).
// Points are named by their index in the chunk's pool [N proofs | the chunk's distinct commitments | 64 setup points].
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ckzg {

constexpr uint32_t CELL_GROUPS_NO_POINT = 0xffffffffu;   // a padding term: the point at infinity, scalar 0

struct CellGroupsPlan {
    size_t N = 0, G = 0, P = 0, R = 0, total = 0;   // cells, groups, pairs, rows, terms of all jobs (padded)
    bool quad = false;                              // jobs padded to 8 terms (four-lane ladders) or to 32
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
    std::vector<uint32_t> term_src;                 // [total] pool index of each term's point, or CELL_GROUPS_NO_POINT
    std::vector<uint32_t> part_off;                 // [2 G + 1] first partial of each job (A_0, B_0, A_1, ...)
    size_t per() const { return quad ? 8 : 32; }
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
    std::vector<uint32_t> seen_c(num_commits, CELL_GROUPS_NO_POINT), slot_c(num_commits, 0);
    uint32_t seen_col[128], slot_col[128];
    for (int c = 0; c < 128; c++) seen_col[c] = CELL_GROUPS_NO_POINT;
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
    auto padded = [](size_t n, size_t per) { return (n + per - 1) / per * per; };
    size_t total8 = 0;
    for (size_t g = 0; g < G; g++) {
        const size_t n = (size_t)(start[g + 1] - start[g]), nc = p.pair_off[g + 1] - p.pair_off[g];
        if (n) total8 += padded(nc + n + 64, 8) + padded(n, 8);
    }
    p.quad = total8 <= quad_max_terms;
    const size_t per = p.per();
    p.gd.assign(4 * G + 1, 0);
    p.part_off.assign(2 * G + 1, 0);
    p.pair_term.resize(P);
    p.term_src.clear();
    uint32_t *gstart = p.gd.data(), *term_a = gstart + G + 1, *ncs = term_a + G, *term_b = ncs + G;
    const uint32_t pool_commit = (uint32_t)N, pool_setup = (uint32_t)(N + num_commits);
    for (size_t g = 0; g < G; g++) {
        const size_t a = (size_t)start[g], n = (size_t)(start[g + 1] - start[g]), nc = p.pair_off[g + 1] - p.pair_off[g];
        gstart[g] = (uint32_t)a;
        ncs[g] = (uint32_t)nc;
        term_a[g] = (uint32_t)p.term_src.size();
        p.part_off[2 * g] = (uint32_t)(p.term_src.size() / per);
        if (n) {
            for (size_t j = 0; j < nc; j++) {
                p.pair_term[p.pair_off[g] + j] = (uint32_t)p.term_src.size();
                p.term_src.push_back(pool_commit + p.pair_commit[p.pair_off[g] + j]);
            }
            for (size_t i = 0; i < n; i++) p.term_src.push_back((uint32_t)(a + i));
            for (uint32_t k = 0; k < 64; k++) p.term_src.push_back(pool_setup + k);
            p.term_src.resize(padded(p.term_src.size(), per), CELL_GROUPS_NO_POINT);
        }
        term_b[g] = (uint32_t)p.term_src.size();
        p.part_off[2 * g + 1] = (uint32_t)(p.term_src.size() / per);
        if (n) {
            for (size_t i = 0; i < n; i++) p.term_src.push_back((uint32_t)(a + i));
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
