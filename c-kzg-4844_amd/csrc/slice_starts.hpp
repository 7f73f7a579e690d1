// The start array of a call that takes many slices of flat arrays at once (groups of cells, groups of blobs, rows of
// cells): slice i is [start[i], start[i + 1]).  Plain C++ (no HIP).
#pragma once
#include <cstdint>

namespace ckzg {

// start: n + 1 entries, starts at 0, does not decrease
inline bool slice_starts_ok(const uint64_t *start, uint64_t n) {
    if (!start || start[0] != 0) return false;
    for (uint64_t i = 0; i < n; i++) {
        if (start[i + 1] < start[i]) return false;
    }
    return true;
}

}  // namespace ckzg
