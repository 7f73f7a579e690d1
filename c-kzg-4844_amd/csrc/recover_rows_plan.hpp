// Index maps of ckzg_hip_recover_cells_and_kzg_proofs_rows: which rows of the call are valid, which distinct sets of
// cells they hold, and where every cell of a chunk lands on the device.  Plain C++ (no HIP, no field arithmetic):
// host_shim.cpp exposes the same maps to the CPU tests (tests/test_recover_rows_cpu.py).
//
// The call is num_rows rows over flat cell_indices[] / cells[]; row r is the slice [row_start[r], row_start[r + 1]).
// A row is valid as recover_cells_and_kzg_proofs takes it (eip7594.c:191-213): 64..128 cells, every index < 128,
// indices strictly ascending.  Valid rows get device rows in caller order, at most chunk_rows per chunk; an invalid
// row gets none (it costs no copy and no kernel) and a chunk never cuts a row.  Per chunk:
//   row_caller  device row -> caller row;
//   row_set     device row -> id of its set: the 128-bit mask of the cells it holds, deduplicated inside the chunk
//               through a hash map (ids in order of first appearance);
//   set_mask    4 words per set, bit c of word c / 32 = cell c is held (the missing cells are the zeros);
//   cell_dst    for every cell the chunk copies, in copy order: device row * 128 + column -- the scatter's target;
//   runs        maximal runs of consecutive valid caller rows: one host-to-device copy of their cells each (they are
//               contiguous in the caller's array) and one copy back of their outputs.
#pragma once
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "slice_starts.hpp"

namespace ckzg {

struct RecoverRowsRun {
    uint64_t caller_row, src_cell;   // first caller row of the run, its first cell in the caller's flat arrays
    uint32_t dev_row, dev_cell;      // first device row, first cell of the chunk's device input
    uint32_t rows, cells;
};

struct RecoverRowsChunk {
    std::vector<uint64_t> row_caller;
    std::vector<uint32_t> row_set, set_mask, cell_dst;
    std::vector<RecoverRowsRun> runs;
    bool all_full = true;            // every row holds all 128 cells: nothing to recover, the proofs only
    size_t rows() const { return row_caller.size(); }
    size_t sets() const { return set_mask.size() / 4; }
    size_t cells() const { return cell_dst.size(); }
};

struct RecoverRowsPlan {
    std::vector<uint8_t> valid;              // [num_rows]
    std::vector<RecoverRowsChunk> chunks;
    bool any_invalid = false;
    size_t max_rows = 0, max_cells = 0, max_sets = 0;   // over the chunks: what the device buffers must hold
};

struct RecoverRowsMaskHash {
    size_t operator()(const std::pair<uint64_t, uint64_t> &m) const {
        uint64_t h = m.first * 0x9e3779b97f4a7c15ull ^ (m.second + 0x632be59bd9b4e019ull);
        h ^= h >> 29;
        h *= 0xbf58476d1ce4e5b9ull;
        return (size_t)(h ^ (h >> 32));
    }
};

// row_start must have passed slice_starts_ok
inline void build_recover_rows_plan(RecoverRowsPlan &p, const uint64_t *cell_indices, const uint64_t *row_start,
                                    uint64_t num_rows, size_t chunk_rows) {
    p.valid.assign((size_t)num_rows, 0);
    p.chunks.clear();
    p.any_invalid = false;
    p.max_rows = p.max_cells = p.max_sets = 0;
    if (chunk_rows == 0) chunk_rows = 1;
    std::unordered_map<std::pair<uint64_t, uint64_t>, uint32_t, RecoverRowsMaskHash> ids;
    RecoverRowsChunk *ch = nullptr;
    auto close = [&]() {
        if (!ch) return;
        if (ch->rows() > p.max_rows) p.max_rows = ch->rows();
        if (ch->cells() > p.max_cells) p.max_cells = ch->cells();
        if (ch->sets() > p.max_sets) p.max_sets = ch->sets();
        ch = nullptr;
    };
    bool prev_valid = false;
    for (uint64_t r = 0; r < num_rows; r++) {
        const uint64_t a = row_start[r], n = row_start[r + 1] - a;
        uint64_t m[2] = {0, 0};
        bool ok = n >= 64 && n <= 128;
        for (uint64_t i = 0; ok && i < n; i++) {
            const uint64_t c = cell_indices[a + i];
            if (c >= 128 || (i > 0 && c <= cell_indices[a + i - 1])) ok = false;
            else m[c >> 6] |= (uint64_t)1 << (c & 63);
        }
        p.valid[(size_t)r] = ok ? 1 : 0;
        if (!ok) {
            p.any_invalid = true;
            prev_valid = false;
            continue;
        }
        if (ch && ch->rows() == chunk_rows) close();
        if (!ch) {
            p.chunks.emplace_back();
            ch = &p.chunks.back();
            ids.clear();
            prev_valid = false;
        }
        const uint32_t dev_row = (uint32_t)ch->rows(), dev_cell = (uint32_t)ch->cells();
        auto it = ids.find({m[0], m[1]});
        if (it == ids.end()) {
            it = ids.emplace(std::make_pair(m[0], m[1]), (uint32_t)ch->sets()).first;
            for (int w = 0; w < 4; w++) ch->set_mask.push_back((uint32_t)(m[w >> 1] >> (32 * (w & 1))));
        }
        ch->row_caller.push_back(r);
        ch->row_set.push_back(it->second);
        if (n != 128) ch->all_full = false;
        for (uint64_t i = 0; i < n; i++) ch->cell_dst.push_back(dev_row * 128u + (uint32_t)cell_indices[a + i]);
        if (prev_valid) {
            ch->runs.back().rows++;
            ch->runs.back().cells += (uint32_t)n;
        } else {
            ch->runs.push_back(RecoverRowsRun{r, a, dev_row, dev_cell, 1u, (uint32_t)n});
        }
        prev_valid = true;
    }
    close();
}

}  // namespace ckzg
