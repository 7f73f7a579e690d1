// locate_plan.hpp -- which items of a chunk are false, found by bisection over a predicate range_ok(a, b) on contiguous
// ranges (ckzg_hip_verify_kzg_proof_batch_locate / ckzg_hip_verify_blob_kzg_proof_batch_locate /
// ckzg_hip_verify_cell_kzg_proof_batch_locate; DESIGN.md sections 3f, 3g), and the chunk challenges of the point and cell
// forms.  Pure host code, shared by the product (ckzg_api2.hip: the predicate is one two-pairing check over differences
// of prefix sums) and the host test shim (host_shim.cpp: hs_locate_bisect, hs_locate_points_host, hs_locate_cells_host,
// hs_locate_cosets_host).
//
// The rules are fixed, so that the number of checks is a property and not an observation:
//   * invalid items are inert (they contribute infinity to every range) and are settled from their flag: ok = false;
//   * a chunk without a valid item runs no check;
//   * otherwise the root [0, m) is checked; true settles every valid item as true with that one check;
//   * a false range of more than one item is split at a + ceil((b - a) / 2).  The left halves of a level are checked
//     together; where the left half is true the right half is false by inference, without a check; where it is false
//     the right half is checked in a second round of the same level;
//   * a false range of one item, checked or inferred, gives ok = false.
// Hence with f false items among m: checks <= 1 + 2 f ceil(log2 m), and exactly 1 when f = 0.
// Hand-over: before a level starts, if checks done + 2 * (open ranges) would exceed max_checks the bisection stops and
// the open ranges are returned; their items take their verdict elsewhere (the per-lane GPU check).  So checks <=
// max(max_checks, 1): the root check is always run.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ckzg {

struct LocateRange {
    size_t a, b;
};

struct LocateOutcome {
    uint64_t checks = 0;
    std::vector<LocateRange> open;   // unsplit false ranges at hand-over: ok[] of their valid items is not settled (false)
};

// ok[m] out; invalid[m] in (non-zero: settled as false, inert in every range).  range_ok(a, b) -> bool for 0 <= a < b <= m;
// par_for(n, fn) runs fn(0) ... fn(n - 1), in any order and possibly at once: the checks of a round are independent.
template <class RangeOk, class ParFor>
LocateOutcome locate_bisect(bool *ok, const uint8_t *invalid, size_t m, uint64_t max_checks, RangeOk &&range_ok, ParFor &&par_for) {
    LocateOutcome out;
    size_t valid = 0;
    for (size_t i = 0; i < m; i++) {
        ok[i] = false;
        valid += invalid[i] ? 0 : 1;
    }
    if (!valid) return out;
    auto settle_true = [&](const LocateRange &r) {
        for (size_t i = r.a; i < r.b; i++) ok[i] = !invalid[i];
    };
    out.checks = 1;
    if (range_ok((size_t)0, m)) {
        settle_true({0, m});
        return out;
    }
    std::vector<LocateRange> level;   // false ranges of more than one item
    if (m > 1) level.push_back({0, m});
    while (!level.empty()) {
        if (out.checks + 2 * (uint64_t)level.size() > max_checks) {
            out.open = level;
            return out;
        }
        const size_t n = level.size();
        std::vector<uint8_t> left_ok(n), right_ok(n, 0);
        auto mid = [&](size_t j) { return level[j].a + (level[j].b - level[j].a + 1) / 2; };
        par_for(n, [&](size_t j) { left_ok[j] = range_ok(level[j].a, mid(j)) ? 1 : 0; });
        out.checks += n;
        std::vector<size_t> second;   // left half false: the right half is not known
        for (size_t j = 0; j < n; j++)
            if (!left_ok[j]) second.push_back(j);
        par_for(second.size(), [&](size_t t) { right_ok[second[t]] = range_ok(mid(second[t]), level[second[t]].b) ? 1 : 0; });
        out.checks += second.size();
        std::vector<LocateRange> next;
        auto settle = [&](const LocateRange &r, bool is_ok) {
            if (is_ok) settle_true(r);
            else if (r.b - r.a > 1) next.push_back(r);
            // (a false range of one item: ok stays false)
        };
        for (size_t j = 0; j < n; j++) {
            settle({level[j].a, mid(j)}, left_ok[j] != 0);
            settle({mid(j), level[j].b}, right_ok[j] != 0);   // (left true: right_ok is 0, false by inference)
        }
        level.swap(next);
    }
    return out;
}

// The challenge of a chunk of the point form: the digest of the library's batch transcript (eip4844.c:597-680:
// "RCKZGBATCH___V1_" | u64be 4096 | u64be n | (C_i | z_i | y_i | proof_i)*) over the chunk's items as given -- a per-item
// verdict does not depend on r, so an invalid item's bytes may be in it.  Sha: host_pairing.hpp's Sha256.
template <class Sha>
void locate_point_digest(uint8_t digest[32], const uint8_t *c48, const uint8_t *z32, const uint8_t *y32, const uint8_t *p48, uint64_t n) {
    Sha h;
    uint8_t head[32] = {'R', 'C', 'K', 'Z', 'G', 'B', 'A', 'T', 'C', 'H', '_', '_', '_', 'V', '1', '_'};
    for (int i = 0; i < 8; i++) {
        head[16 + i] = (uint8_t)((uint64_t)4096 >> (8 * (7 - i)));
        head[24 + i] = (uint8_t)(n >> (8 * (7 - i)));
    }
    h.update(head, 32);
    for (uint64_t i = 0; i < n; i++) {
        h.update(c48 + 48 * i, 48);
        h.update(z32 + 32 * i, 32);
        h.update(y32 + 32 * i, 32);
        h.update(p48 + 48 * i, 48);
    }
    h.finish(digest);
}

// The challenge of a chunk of the cell form (ckzg_hip_verify_cell_kzg_proof_batch_locate): two levels, so that the
// 2,152 bytes of every item are hashed on their own -- on as many threads as there are -- and only 32 bytes per item
// go through the one stream that binds them together.  Over the chunk's items as given, invalid ones included:
//   leaf_i = SHA-256("CKZGHIPCELLLEAF_" | C_i (48) | u64be cell_index_i | cell_i (2048) | proof_i (48))
//   root   = SHA-256("CKZGHIPCELLROOT_" | u64be 4096 | u64be k | leaf_0 | ... | leaf_{k-1})
// (Not the reference's transcript, eip7594.c:390-482, which is one stream over every cell: a per-item verdict does not
// depend on r.)
template <class Sha>
void locate_cell_leaf(uint8_t leaf[32], const uint8_t *c48, uint64_t cell_index, const uint8_t *cell2048, const uint8_t *p48) {
    Sha h;
    uint8_t head[24] = {'C', 'K', 'Z', 'G', 'H', 'I', 'P', 'C', 'E', 'L', 'L', 'L', 'E', 'A', 'F', '_'};
    h.update(head, 16);
    h.update(c48, 48);
    for (int i = 0; i < 8; i++) head[i] = (uint8_t)(cell_index >> (8 * (7 - i)));
    h.update(head, 8);
    h.update(cell2048, 2048);
    h.update(p48, 48);
    h.finish(leaf);
}
template <class Sha>
void locate_cell_root(uint8_t digest[32], const uint8_t *leaves, uint64_t k) {
    Sha h;
    uint8_t head[32] = {'C', 'K', 'Z', 'G', 'H', 'I', 'P', 'C', 'E', 'L', 'L', 'R', 'O', 'O', 'T', '_'};
    for (int i = 0; i < 8; i++) {
        head[16 + i] = (uint8_t)((uint64_t)4096 >> (8 * (7 - i)));
        head[24 + i] = (uint8_t)(k >> (8 * (7 - i)));
    }
    h.update(head, 32);
    h.update(leaves, 32 * k);
    h.finish(digest);
}
// both levels on one thread (the host test shim; the product hashes the leaves on its pool)
template <class Sha>
void locate_cell_digest(uint8_t digest[32], const uint8_t *c48, const uint64_t *cell_indices, const uint8_t *cells, const uint8_t *p48,
                        uint64_t k) {
    std::vector<uint8_t> leaves(32 * (k ? k : 1));
    for (uint64_t i = 0; i < k; i++) locate_cell_leaf<Sha>(&leaves[32 * i], c48 + 48 * i, cell_indices[i], cells + 2048 * i, p48 + 48 * i);
    locate_cell_root<Sha>(digest, leaves.data(), k);
}

// The challenge of a chunk of the coset form (ckzg_hip_verify_coset_kzg_proof_batch_locate), items of l = 2^e values:
// the same two levels, with the coset size in every leaf and in the root.
//   leaf_i = SHA-256("CKZGHIPCOSETLEAF" | C_i (48) | u64be l | u64be coset_index_i | its l values (32 l) | proof_i (48))
//   root   = SHA-256("CKZGHIPCOSETROOT" | u64be 4096 | u64be l | u64be k | leaf_0 | ... | leaf_{k-1})
template <class Sha>
void locate_coset_leaf(uint8_t leaf[32], const uint8_t *c48, uint64_t coset_index, const uint8_t *values, const uint8_t *p48, int e) {
    const uint64_t l = (uint64_t)1 << e;
    Sha h;
    uint8_t head[16] = {'C', 'K', 'Z', 'G', 'H', 'I', 'P', 'C', 'O', 'S', 'E', 'T', 'L', 'E', 'A', 'F'};
    h.update(head, 16);
    h.update(c48, 48);
    for (int i = 0; i < 8; i++) {
        head[i] = (uint8_t)(l >> (8 * (7 - i)));
        head[8 + i] = (uint8_t)(coset_index >> (8 * (7 - i)));
    }
    h.update(head, 16);
    h.update(values, 32 * l);
    h.update(p48, 48);
    h.finish(leaf);
}
template <class Sha>
void locate_coset_root(uint8_t digest[32], const uint8_t *leaves, uint64_t k, int e) {
    const uint64_t l = (uint64_t)1 << e;
    Sha h;
    uint8_t head[40] = {'C', 'K', 'Z', 'G', 'H', 'I', 'P', 'C', 'O', 'S', 'E', 'T', 'R', 'O', 'O', 'T'};
    for (int i = 0; i < 8; i++) {
        head[16 + i] = (uint8_t)((uint64_t)4096 >> (8 * (7 - i)));
        head[24 + i] = (uint8_t)(l >> (8 * (7 - i)));
        head[32 + i] = (uint8_t)(k >> (8 * (7 - i)));
    }
    h.update(head, 40);
    h.update(leaves, 32 * k);
    h.finish(digest);
}
// both levels on one thread (the host test shim; the product hashes the leaves on its pool)
template <class Sha>
void locate_coset_digest(uint8_t digest[32], const uint8_t *c48, const uint64_t *coset_indices, const uint8_t *evals, const uint8_t *p48,
                         uint64_t k, int e) {
    std::vector<uint8_t> leaves(32 * (k ? k : 1));
    for (uint64_t i = 0; i < k; i++)
        locate_coset_leaf<Sha>(&leaves[32 * i], c48 + 48 * i, coset_indices[i], evals + ((size_t)(32 * i) << e), p48 + 48 * i, e);
    locate_coset_root<Sha>(digest, leaves.data(), k, e);
}

}  // namespace ckzg
