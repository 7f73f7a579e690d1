// coset_locate_plan.hpp -- the launch decisions of ckzg_hip_verify_coset_kzg_proof_batch_locate (ckzg_api2.hip:
// locate_cosets_on), once, for the host function and, through libhost_shim.so, for the CPU tests
// (tests/test_coset_locate_cpu.py restates them in Python).  The index arithmetic is coset_verify_plan.hpp's.
#pragma once
#include <cstdint>

#include "g1_fft_plan.hpp"

namespace ckzg {

// A chunk holds at most this many values (slots), and never more items than a chunk of the point form: 65,536 items at
// e <= 4, 32,768 at e = 5, 16,384 at e = 6 (the chunk of the cell form).
constexpr uint64_t COSET_LOCATE_CHUNK_SLOTS = 1048576;
constexpr uint64_t COSET_LOCATE_CHUNK_ITEMS_MAX = 65536;
HD uint64_t coset_locate_chunk_items(int e) {
    const uint64_t by_slots = COSET_LOCATE_CHUNK_SLOTS >> e;
    return by_slots < COSET_LOCATE_CHUNK_ITEMS_MAX ? by_slots : COSET_LOCATE_CHUNK_ITEMS_MAX;
}

// Several devices: no shard below this many items (the cell form's figure: an item's cost is its two ladders)
constexpr uint64_t COSET_LOCATE_MIN_SHARD = 64;

// The fixed-base sum -[I_i(s)]_1 of an item has 2^e terms of nwin digits each; k_msm_small<LPV> gives a vector LPV lanes
// of a 64-lane workgroup.  One wave per vector (LPV = 64) is the latency form: below COSET_LOCATE_SUM_WAVE_BELOW[e]
// items it is launched whatever it idles, because the chip is not full anyway; from there on a vector gets
// COSET_LOCATE_SUM_LPV[e] lanes.  Both rows are measured (tools/bench_coset_locate.py --sum-forms;
// profiles/coset_locate_bench.json, "sum_forms": the kernel alone, medians of 20, items in powers of two from 128 to
// 8,192): LPV[e] is the form that is fastest at 8,192 items, WAVE_BELOW[e] the first measured count at which that form's
// median is below the wave form's.  The wave form wins at every e up to 1,024 items (0.06 against 0.11 ms at e = 0, 0.40
// against 1.06 ms at e = 6); at 8,192 the narrow form is 0.13 against 0.31 ms at e = 0 and 2.02 against 2.25 ms at e = 6.
// One narrow form per e is a simplification that costs at most 0.07 ms (e = 4 at 4,096 items: 16 lanes would take 0.41 ms,
// the wave form takes 0.49) of a call of 12 ms and more.
constexpr uint32_t COSET_LOCATE_SUM_WAVE_BELOW[COSET_MAX_LOG + 1] = {2048, 2048, 4096, 4096, 8192, 8192, 4096};
constexpr int COSET_LOCATE_SUM_LPV[COSET_MAX_LOG + 1] = {4, 8, 8, 8, 8, 8, 16};
HD int coset_locate_sum_lpv(int e, uint64_t items) {
    return items < COSET_LOCATE_SUM_WAVE_BELOW[e] ? 64 : COSET_LOCATE_SUM_LPV[e];
}

}  // namespace ckzg
