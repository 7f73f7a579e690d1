// fk20_fft_plan.hpp -- which form the two length-128 G1 transforms of FK20 (fk20.hip: fk20_fft_stage_enqueue) take for
// a batch of n transforms.  A pure function of its arguments, so that the CPU tests reach it through libhost_shim.so
// (hs_fk20_fft_form) and fk20_layout, the stage function and the launch code read the same decision.
//
// Hand-over points (same-box A/Bs: profiles/r05_fk20_small_ab.txt, profiles/r02_quad_ab.txt).  Radix-8 steps while a
// step's waves fit the chip about once (<= 48 transforms: 1008 waves): with the three-wave ladder and two twiddles per
// workgroup while its 168 workgroups have a compute unit each (<= 8), with the two-wave ladder while the 21 workgroups
// per transform and step mostly find a SIMD per wave (<= 16: 336 workgroups), with the one-wave quad ladder above.
// Radix-4 pairs win up to ~100 transforms and tie with the radix-2 four-lane form up to ~200 (<= 128).  Radix-2 stages
// beyond: four lanes per butterfly while that is at most ~two waves per SIMD (<= 512), one lane per butterfly above.
#pragma once
#include <cstdint>

namespace ckzg {

enum Fk20FftForm {
    FK20_FFT_R8_PIPE_TWO = 0,   // radix-8, three-wave ladder, two twiddles per workgroup (k_g1_fft_r8_ladder_pipe, two = 1)
    FK20_FFT_R8_PIPE = 1,       // radix-8, two-wave ladder (k_g1_fft_r8_ladder_pipe2)
    FK20_FFT_R8_ONE = 2,        // radix-8, one-wave quad ladder with the whole register file (k_g1_fft_r8_ladder_full)
    FK20_FFT_R4 = 3,            // radix-4 pairs (k_g1_fft_r4_ladder, k_g1_fft_r4_post)
    FK20_FFT_R2_QUAD = 4,       // radix-2, four lanes per butterfly (k_g1_fft_twiddle_quad)
    FK20_FFT_R2_LANE = 5,       // radix-2, one lane per butterfly (k_g1_fft_twiddle)
    FK20_FFT_FORMS = 6
};

// the largest batch of each form but the last
struct Fk20FftLimits {
    uint64_t r8_two_max = 8, r8_pipe_max = 16, r8_max = 48, r4_max = 128, quad_max = 512;
};

inline int fk20_fft_form(uint64_t n, const Fk20FftLimits &lim = Fk20FftLimits()) {
    if (n <= lim.r8_max) {
        if (n > lim.r8_pipe_max) return FK20_FFT_R8_ONE;
        return n <= lim.r8_two_max ? FK20_FFT_R8_PIPE_TWO : FK20_FFT_R8_PIPE;
    }
    if (n <= lim.r4_max) return FK20_FFT_R4;
    return n <= lim.quad_max ? FK20_FFT_R2_QUAD : FK20_FFT_R2_LANE;
}

inline bool fk20_fft_is_r8(int form) { return form <= FK20_FFT_R8_ONE; }

// The stage's scratch for n transforms in a given form (offsets from its base, every buffer rounded up to 256 bytes).
// Radix-8: two buffers of n x 128 raw records (g1_pipe.hpp) and n x FK20_R8_LADDERS ladder results; radix-4: n x 128
// points (the post kernel cannot write in place) and n x FK20_R4_LADDERS ladder results; radix-2 works in place.
constexpr uint64_t FK20_POINT_BYTES = 192;      // sizeof(G1XYZZ)
constexpr uint64_t FK20_RAW_BYTES = 57 * 4;     // quad::RAW_WORDS words (fk20.hip asserts both)
constexpr int FK20_R4_LADDERS = 32 * 5;         // per transform and radix-4 step: 32 groups of four points, five ladders each
constexpr int FK20_R8_PER_GROUP = 21;
constexpr int FK20_R8_LADDERS = 16 * FK20_R8_PER_GROUP;   // per transform and radix-8 step: 16 groups of eight points

struct Fk20FftScratchPlan {
    uint64_t a = 0, b = 0, lad = 0;   // radix-8: raw buffers a, b and the ladder results; radix-4: a = tmp, lad
    uint64_t bytes = 0;
};

inline uint64_t fk20_fft_align(uint64_t v) { return (v + 255) / 256 * 256; }

inline Fk20FftScratchPlan fk20_fft_scratch_plan(uint64_t n, int form) {
    Fk20FftScratchPlan p;
    if (fk20_fft_is_r8(form)) {
        p.a = 0;
        p.b = p.a + fk20_fft_align(n * 128 * FK20_RAW_BYTES);
        p.lad = p.b + fk20_fft_align(n * 128 * FK20_RAW_BYTES);
        p.bytes = p.lad + fk20_fft_align(n * FK20_R8_LADDERS * FK20_RAW_BYTES);
    } else if (form == FK20_FFT_R4) {
        p.a = 0;
        p.lad = p.a + fk20_fft_align(n * 128 * FK20_POINT_BYTES);
        p.bytes = p.lad + fk20_fft_align(n * FK20_R4_LADDERS * FK20_POINT_BYTES);
    }
    return p;
}

}  // namespace ckzg
