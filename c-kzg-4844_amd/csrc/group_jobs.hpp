// The job layout the grouped verifications share (coset_groups_plan.hpp, blob_groups_plan.hpp): two linear
// combinations per group, A_g then B_g, laid out job after job for ONE pass of the ladder kernels
// (lincomb_multi_device).  Every job is padded to a whole partial of those kernels -- 8 terms while all jobs together
// stay within quad_max_terms (the four-lane ladders), 32 otherwise -- and the whole layout to a multiple of 64 terms.
// An empty group has two empty jobs (the empty sum: infinity).  Which points and scalars a job holds is its plan's
// business.  Plain C++ (no HIP), as the plans are.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>


namespace ckzg {

constexpr uint32_t GROUP_JOBS_NO_POINT = 0xffffffffu;   // a padding term: the point at infinity, scalar 0

struct GroupJobs {
    size_t total = 0;                 // terms of all jobs (padded)
    bool quad = false;                // jobs padded to 8 terms (four-lane ladders) or to 32
    std::vector<uint32_t> term_src;   // [total] index of each term's point in the plan's pool, or GROUP_JOBS_NO_POINT
    std::vector<uint32_t> part_off;   // [2 G + 1] first partial of each job (A_0, B_0, A_1, ...)
    size_t per() const { return quad ? 8 : 32; }
};

// What a plan appends a job's terms through
struct GroupJobTerms {
    std::vector<uint32_t> &term_src;
    uint32_t at() const { return (uint32_t)term_src.size(); }   // the index the next term gets
    void put(uint32_t src) { term_src.push_back(src); }
};

// count(g, b) -> the number of terms of A_g (b = false) or B_g (b = true), 0 for both in an empty group;
// emit(g, b, GroupJobTerms &) appends them.  term_a / term_b [G] receive the first term of each job.
template <class Count, class Emit>
inline void lay_out_group_jobs(GroupJobs &j, size_t G, size_t quad_max_terms, uint32_t *term_a, uint32_t *term_b, Count count,
                               Emit emit) {
    auto padded = [](size_t n, size_t per) { return (n + per - 1) / per * per; };
    size_t total8 = 0;
    for (size_t g = 0; g < G; g++) total8 += padded(count(g, false), 8) + padded(count(g, true), 8);
    j.quad = total8 <= quad_max_terms;
    const size_t per = j.per();
    j.part_off.assign(2 * G + 1, 0);
    j.term_src.clear();
    GroupJobTerms out{j.term_src};
    for (size_t g = 0; g < G; g++) {
        for (int b = 0; b < 2; b++) {
            (b ? term_b : term_a)[g] = out.at();
            j.part_off[2 * g + b] = (uint32_t)(j.term_src.size() / per);
            emit(g, b != 0, out);
            j.term_src.resize(padded(j.term_src.size(), per), GROUP_JOBS_NO_POINT);
        }
    }
    j.part_off[2 * G] = (uint32_t)(j.term_src.size() / per);
    // the ladder kernels take a multiple of 64 terms
    j.term_src.resize(padded(j.term_src.size(), 64), GROUP_JOBS_NO_POINT);
    j.total = j.term_src.size();
}

}  // namespace ckzg
