// Index maps of recovery by rows (ckzg_hip_recover_cosets_and_kzg_proofs_rows, and ckzg_hip_recover_cells_and_kzg_proofs_rows
// at e = 6): which rows of the call are valid, which distinct sets of cosets they hold, and where every coset of a chunk
// lands on the device.  Plain C++ (no HIP, no field arithmetic): host_shim.cpp exposes the same maps to the CPU tests
// (tests/test_coset_recover_cpu.py, whose model is tests/coset_recover_expect.py; tests/test_recover_rows_cpu.py).
//
// Coset size l = 2^e, e <= 6; a row has m = 8192 >> e cosets.  The call is num_rows rows over flat coset_indices[] /
// evals[]; row r is the slice [row_start[r], row_start[r + 1]).  A row is valid with m/2 .. m cosets, every index < m,
// indices strictly ascending.  Valid rows get device rows in caller order, at most chunk_rows per chunk; an invalid row
// gets none and a chunk never cuts a row.  Per chunk:
//   row_caller  device row -> caller row;
//   row_set     device row -> id of its set: the m-bit mask of the cosets it holds (m / 32 words, up to 1 KB),
//               deduplicated inside the chunk through a hash of the words, compared word by word on collision (ids in
//               order of first appearance);
//   set_mask    m / 32 words per set, bit c of word c / 32 = coset c is held;
//   coset_dst   for every coset the chunk copies, in copy order: device row * m + c -- the scatter's target;
//   runs        maximal runs of consecutive valid caller rows: one copy in and one copy back each;
//   miss        for every set, back to back, the index into roots_of_unity of w_m^brp_{13-e}(j) = l * brp_{13-e}(j) for
//               each missing coset j in ascending j (the kernel does no bit reversal per factor); set s owns
//               miss[miss_start[s] .. miss_start[s + 1]).
#pragma once
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "slice_starts.hpp"

namespace ckzg {

constexpr uint32_t COSET_RECOVER_EXT = 8192;
constexpr int COSET_RECOVER_MAX_LOG = 6;

constexpr uint32_t coset_recover_cosets(int e) { return COSET_RECOVER_EXT >> e; }
constexpr uint32_t coset_recover_mask_words(int e) { return coset_recover_cosets(e) / 32; }   // m >= 128
// brp_{13-e}(c), c < m: the 32-bit reversal (halves, bytes, nibbles, pairs, bits), shifted down
constexpr uint32_t coset_recover_brp(uint32_t c, int e) {
    c = (c >> 16) | (c << 16);
    c = ((c & 0xff00ff00u) >> 8) | ((c & 0x00ff00ffu) << 8);
    c = ((c & 0xf0f0f0f0u) >> 4) | ((c & 0x0f0f0f0fu) << 4);
    c = ((c & 0xccccccccu) >> 2) | ((c & 0x33333333u) << 2);
    c = ((c & 0xaaaaaaaau) >> 1) | ((c & 0x55555555u) << 1);
    return c >> (19 + e);
}

// ---- the factor launch: `parts` lanes share the product of one coset (constexpr: the kernel calls these too) ----
// One lane per (coset, part); a part takes a contiguous slice of the set's missing list.  The aim is a launch of about
// one wave per SIMD (COSET_RECOVER_FILL_WAVES: 256 CUs x 4) without a slice of the longest list (m / 2 factors) falling
// below COSET_RECOVER_MIN_CHAIN: a shorter chain no longer hides the fold over the parts and the inversion behind it.
// Returns a power of two; 1 where sets * m lanes already fill the chip.
constexpr uint32_t COSET_RECOVER_FILL_WAVES = 1024;
constexpr uint32_t COSET_RECOVER_MIN_CHAIN = 32;
constexpr uint32_t COSET_RECOVER_THREADS = 256;   // at most; a workgroup holds every part of its cosets
constexpr uint32_t coset_recover_parts(size_t sets, int e) {
    const uint64_t m = coset_recover_cosets(e);
    uint32_t parts = 1;
    while ((uint64_t)sets * m * parts / 64 < COSET_RECOVER_FILL_WAVES && (m / 2) / (2 * parts) >= COSET_RECOVER_MIN_CHAIN)
        parts <<= 1;
    return parts;
}
// every slice has this many steps (the loop is uniform over a workgroup); part q owns the missing-list positions
// [q * len, min((q + 1) * len, count)), the steps beyond are the factor 1
constexpr uint32_t coset_recover_slice_len(uint32_t count, uint32_t parts) { return (count + parts - 1) / parts; }
constexpr uint32_t coset_recover_slice_valid(uint32_t count, uint32_t parts, uint32_t q) {
    const uint64_t len = coset_recover_slice_len(count, parts), lo = q * len;
    return lo >= count ? 0u : (uint32_t)(count - lo < len ? count - lo : len);
}
// lanes of a workgroup and workgroups per set: block / parts cosets per workgroup
constexpr uint32_t coset_recover_block(int e, uint32_t parts) {
    const uint64_t items = (uint64_t)coset_recover_cosets(e) * parts;
    return items < COSET_RECOVER_THREADS ? (uint32_t)items : COSET_RECOVER_THREADS;
}

struct CosetRecoverRun {
    uint64_t caller_row, src_coset;   // first caller row of the run, its first coset in the caller's flat arrays
    uint32_t dev_row, dev_coset;      // first device row, first coset of the chunk's device input
    uint32_t rows, cosets;
};

struct CosetRecoverChunk {
    std::vector<uint64_t> row_caller;
    std::vector<uint32_t> row_set, set_mask, coset_dst, miss, miss_start;
    std::vector<CosetRecoverRun> runs;
    bool all_full = true;             // every row holds all m cosets: nothing to recover, the proofs only
    size_t rows() const { return row_caller.size(); }
    size_t sets() const { return miss_start.empty() ? 0 : miss_start.size() - 1; }
    size_t cosets() const { return coset_dst.size(); }
};

struct CosetRecoverPlan {
    int e = 0;
    std::vector<uint8_t> valid;       // [num_rows]
    std::vector<CosetRecoverChunk> chunks;
    bool any_invalid = false;
    size_t max_rows = 0, max_cosets = 0, max_sets = 0, max_miss = 0;   // over the chunks: what the device buffers must hold
};

inline uint64_t coset_recover_mask_hash(const uint32_t *w, size_t n) {
    uint64_t h = 0x632be59bd9b4e019ull;
    for (size_t i = 0; i < n; i++) {
        h = (h ^ w[i]) * 0x9e3779b97f4a7c15ull;
        h ^= h >> 29;
    }
    return h;
}

// the missing list of one set, appended to `miss`: mask as set_mask holds it (m / 32 words)
inline void coset_recover_missing(std::vector<uint32_t> &miss, const uint32_t *mask, int e) {
    const size_t at = miss.size();
    miss.resize(at + coset_recover_cosets(e));   // room for every coset, cut back below: no growth check per entry
    uint32_t *out = miss.data() + at;
    for (uint32_t w = 0; w < coset_recover_mask_words(e); w++)
        for (uint32_t z = ~mask[w]; z; z &= z - 1) *out++ = coset_recover_brp(32 * w + (uint32_t)__builtin_ctz(z), e) << e;
    miss.resize((size_t)(out - miss.data()));
}

// row_start must have passed slice_starts_ok; e <= COSET_RECOVER_MAX_LOG
inline void build_coset_recover_plan(CosetRecoverPlan &p, const uint64_t *coset_indices, const uint64_t *row_start,
                                     uint64_t num_rows, int e, size_t chunk_rows) {
    const uint32_t m = coset_recover_cosets(e), W = coset_recover_mask_words(e);
    p.e = e;
    p.valid.assign((size_t)num_rows, 0);
    p.chunks.clear();
    p.any_invalid = false;
    p.max_rows = p.max_cosets = p.max_sets = p.max_miss = 0;
    if (chunk_rows == 0) chunk_rows = 1;
    std::unordered_multimap<uint64_t, uint32_t> ids;   // hash of the mask -> set id
    std::vector<uint32_t> mask(W);
    CosetRecoverChunk *ch = nullptr;
    auto close = [&]() {
        if (!ch) return;
        if (ch->rows() > p.max_rows) p.max_rows = ch->rows();
        if (ch->cosets() > p.max_cosets) p.max_cosets = ch->cosets();
        if (ch->sets() > p.max_sets) p.max_sets = ch->sets();
        if (ch->miss.size() > p.max_miss) p.max_miss = ch->miss.size();
        ch = nullptr;
    };
    bool prev_valid = false;
    for (uint64_t r = 0; r < num_rows; r++) {
        const uint64_t a = row_start[r], n = row_start[r + 1] - a;
        bool ok = n >= m / 2 && n <= m;
        mask.assign(W, 0);
        for (uint64_t i = 0; ok && i < n; i++) {
            const uint64_t c = coset_indices[a + i];
            if (c >= m || (i > 0 && c <= coset_indices[a + i - 1])) ok = false;
            else mask[c >> 5] |= 1u << (c & 31);
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
            ch->miss_start.push_back(0);
            ids.clear();
            prev_valid = false;
        }
        const uint32_t dev_row = (uint32_t)ch->rows(), dev_coset = (uint32_t)ch->cosets();
        const uint64_t h = coset_recover_mask_hash(mask.data(), W);
        uint32_t set = 0xffffffffu;
        auto range = ids.equal_range(h);
        for (auto it = range.first; it != range.second && set == 0xffffffffu; ++it) {
            const uint32_t *have = ch->set_mask.data() + (size_t)it->second * W;
            bool same = true;
            for (uint32_t w = 0; same && w < W; w++) same = have[w] == mask[w];
            if (same) set = it->second;
        }
        if (set == 0xffffffffu) {
            set = (uint32_t)ch->sets();
            ids.emplace(h, set);
            ch->set_mask.insert(ch->set_mask.end(), mask.begin(), mask.end());
            coset_recover_missing(ch->miss, mask.data(), e);
            ch->miss_start.push_back((uint32_t)ch->miss.size());
        }
        ch->row_caller.push_back(r);
        ch->row_set.push_back(set);
        if (n != m) ch->all_full = false;
        for (uint64_t i = 0; i < n; i++) ch->coset_dst.push_back(dev_row * m + (uint32_t)coset_indices[a + i]);
        if (prev_valid) {
            ch->runs.back().rows++;
            ch->runs.back().cosets += (uint32_t)n;
        } else {
            ch->runs.push_back(CosetRecoverRun{r, a, dev_row, dev_coset, 1u, (uint32_t)n});
        }
        prev_valid = true;
    }
    close();
}

}  // namespace ckzg
