// Planning of the repair pass of ckzg_hip_repair_cosets_and_kzg_proofs_rows (and ckzg_hip_repair_cells_and_kzg_proofs_rows
// at e = 6): the verdict of a row from its flags, which rows go to the locate pipeline and as which flat items, which of
// their cosets survive it, the rows of the second recovery pass and where their outputs land, the final verdicts.
// Plain C++ (no HIP, no field arithmetic): host_shim.cpp exposes it to tests/test_coset_repair_cpu.py, whose model is
// tests/coset_repair_expect.py.
//
// Coset size l = 2^e, e <= 6; a row has m = 8192 >> e cosets and is recoverable from m / 2 of them.  Row r of the call
// is the slice [row_start[r], row_start[r + 1]) of the caller's flat arrays.  The first pass leaves three flags a row:
// invalid (status[r] != 0), high (coefficients 4096 .. 8191 not all zero: the held cosets lie on no polynomial of degree
// < 4096) and mismatch (the commitment of the recovered blob is not the given one; never set without commitments).
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace ckzg {

// (the values of CKZG_HIP_ROW_* in ckzg_hip.h; ckzg_api2.hip asserts that they are)
enum CosetRepairVerdict : uint8_t {
    COSET_ROW_OK = 0,
    COSET_ROW_INCONSISTENT = 1,
    COSET_ROW_MISMATCH = 2,
    COSET_ROW_REPAIRED = 3,
    COSET_ROW_UNRECOVERABLE = 4,
    COSET_ROW_INVALID = 5,
};

constexpr uint32_t coset_repair_cosets(int e) { return 8192u >> e; }

// precedence: INVALID, then INCONSISTENT, then MISMATCH, then OK
constexpr uint8_t coset_repair_first_verdict(bool invalid, bool high, bool mismatch) {
    return invalid ? COSET_ROW_INVALID : high ? COSET_ROW_INCONSISTENT : mismatch ? COSET_ROW_MISMATCH : COSET_ROW_OK;
}
// a row of the second pass: it must now be consistent AND the committed blob
constexpr uint8_t coset_repair_second_verdict(bool high, bool mismatch) {
    return high || mismatch ? COSET_ROW_UNRECOVERABLE : COSET_ROW_REPAIRED;
}
constexpr bool coset_repair_wants_locate(uint8_t verdict) {
    return verdict == COSET_ROW_INCONSISTENT || verdict == COSET_ROW_MISMATCH;
}

// The verdicts of the first pass over caller rows [lo, hi), and (coset_ok may be null) what they say about the held
// cosets before any pairing: an OK row's are all true -- the checks imply it -- and everything else is false until the
// locate pass has spoken (an INVALID row's stay false).
inline void coset_repair_first_pass(uint8_t *verdict, bool *coset_ok, const uint8_t *status, const uint8_t *high,
                                    const uint8_t *mismatch, const uint64_t *row_start, uint64_t lo, uint64_t hi) {
    for (uint64_t r = lo; r < hi; r++) {
        verdict[r] = coset_repair_first_verdict(status[r] != 0, high[r] != 0, mismatch[r] != 0);
        if (coset_ok)
            for (uint64_t i = row_start[r]; i < row_start[r + 1]; i++) coset_ok[i] = verdict[r] == COSET_ROW_OK;
    }
}

// The locate pass over caller rows [lo, hi): rows with verdict INCONSISTENT or MISMATCH, in caller order, and their held
// cosets as flat items in caller order.  Item i is the caller's coset item_src[i] (index, values, proof) and is paired
// with commitment item_row[i]; row j of `rows` owns the items [item_start[j], item_start[j + 1]).
struct CosetRepairLocate {
    std::vector<uint64_t> rows, item_start, item_src, item_row;
    size_t items() const { return item_src.size(); }
};

inline void coset_repair_locate_plan(CosetRepairLocate &p, const uint8_t *verdict, const uint64_t *row_start, uint64_t lo,
                                     uint64_t hi) {
    p.rows.clear(), p.item_src.clear(), p.item_row.clear();
    p.item_start.assign(1, 0);
    for (uint64_t r = lo; r < hi; r++) {
        if (!coset_repair_wants_locate(verdict[r])) continue;
        p.rows.push_back(r);
        for (uint64_t i = row_start[r]; i < row_start[r + 1]; i++) {
            p.item_src.push_back(i);
            p.item_row.push_back(r);
        }
        p.item_start.push_back(p.item_src.size());
    }
}

// The second pass: every located row that keeps at least m / 2 true cosets becomes one row of a rows call of its own,
// over the flat list `src` of the caller's cosets that verified (ascending inside a row, as the caller gave them).  Row
// j of that call is [row_start[j], row_start[j + 1]) of `src` and its outputs, status and flags land at caller row
// out_row[j].  A located row with fewer true cosets is in `lost`: UNRECOVERABLE without a second pass.
struct CosetRepairSecond {
    std::vector<uint64_t> out_row, row_start, src, lost;
    size_t rows() const { return out_row.size(); }
};

inline void coset_repair_second_plan(CosetRepairSecond &s, const CosetRepairLocate &p, const bool *item_ok, int e) {
    const uint32_t need = coset_repair_cosets(e) / 2;
    s.out_row.clear(), s.src.clear(), s.lost.clear();
    s.row_start.assign(1, 0);
    for (size_t j = 0; j < p.rows.size(); j++) {
        uint64_t good = 0;
        for (uint64_t i = p.item_start[j]; i < p.item_start[j + 1]; i++) good += item_ok[i] ? 1 : 0;
        if (good < need) {
            s.lost.push_back(p.rows[j]);
            continue;
        }
        for (uint64_t i = p.item_start[j]; i < p.item_start[j + 1]; i++)
            if (item_ok[i]) s.src.push_back(p.item_src[i]);
        s.out_row.push_back(p.rows[j]);
        s.row_start.push_back(s.src.size());
    }
}

// what the locate pass said, at the caller's cosets
inline void coset_repair_spread_ok(bool *coset_ok, const CosetRepairLocate &p, const bool *item_ok) {
    for (size_t i = 0; i < p.items(); i++) coset_ok[p.item_src[i]] = item_ok[i];
}

// The final verdicts of the located rows: `lost` rows are UNRECOVERABLE; with the second pass run (high / mismatch now
// hold its flags at the rows' caller places) its rows are REPAIRED or UNRECOVERABLE.
inline void coset_repair_lost(uint8_t *verdict, const CosetRepairSecond &s) {
    for (uint64_t r : s.lost) verdict[r] = COSET_ROW_UNRECOVERABLE;
}
inline void coset_repair_finish(uint8_t *verdict, const CosetRepairSecond &s, const uint8_t *high, const uint8_t *mismatch) {
    for (uint64_t r : s.out_row) verdict[r] = coset_repair_second_verdict(high[r] != 0, mismatch[r] != 0);
}

}  // namespace ckzg
