// g1_fft_plan.hpp -- the host decisions of the general G1 transform (g1_fft.hip; ckzg_hip_g1_fft) and of the one
// openings pipeline behind ckzg_hip_compute_coset_kzg_proofs_batch (every coset of the extended domain) and
// ckzg_hip_compute_domain_kzg_proofs_batch (every domain point: coset size one with a shorter last transform): the
// index maps of a stage, which ladder form runs at which size, how a batch is cut into chunks, where a Toeplitz column
// reads its coefficients and its setup points.  Pure functions of their arguments, so that the CPU tests reach them
// through libhost_shim.so and the kernels use the same maps (HD).
#pragma once
#include <cstddef>
#include <cstdint>

#include "field.hpp"

namespace ckzg {

constexpr int G1_FFT_MAX_LOG = 13;   // the longest transform: the 8192 roots of unity of the setup

// log2(n) for a transform length the library serves (a power of two up to 8192), -1 otherwise
inline int g1_fft_log2(uint64_t n) {
    if (n == 0 || (n & (n - 1)) != 0 || n > ((uint64_t)1 << G1_FFT_MAX_LOG)) return -1;
    int l = 0;
    while (((uint64_t)1 << l) < n) l++;
    return l;
}

// Stage s of a length-2^logn transform (butterfly span 2^s) has n/2 butterflies; those with j = 0 have twiddle 1 and
// need no ladder.  The others are numbered densely, m = 0 .. g1_fft_ladders(logn, s) - 1, group-major:
//   group = m / (half - 1), j = 1 + m % (half - 1), slot of the multiplied point i1 = group * 2^s + half + j,
//   twiddle w_8192^(j * 8192 / 2^s)  (the same exponent whatever n is: w_n^(j n / 2^s)).
HD uint32_t g1_fft_ladders(int logn, int s) { return s < 2 ? 0u : (1u << (logn - 1)) - (1u << (logn - s)); }
HD void g1_fft_ladder_index(uint32_t m, int s, uint32_t &i1, uint32_t &root) {
    const uint32_t half = 1u << (s - 1), per = half - 1u;
    const uint32_t group = m / per, j = 1u + (m - group * per);
    i1 = (group << s) + half + j;
    root = j << (G1_FFT_MAX_LOG - s);
}

// Which ladder form a launch takes.  A half-ladder (one 128-bit GLV half of one product) runs on one lane or on the four
// lanes of a quad (g1_quad.hpp: a 2.3-3x shorter dependent chain for four times the lanes).  The quad form is taken
// while it still leaves the chip under-filled: up to quad_max products per launch, 2 x 4 x 8192 lanes = 1024 waves = one
// wave per SIMD of the 256 compute units at the default.
constexpr uint64_t G1_FFT_QUAD_MAX_DEFAULT = 8192;
enum G1FftForm { G1_FFT_FORM_QUAD = 0, G1_FFT_FORM_LANE = 1 };
inline int g1_fft_form(uint64_t products, uint64_t quad_max) { return products <= quad_max ? G1_FFT_FORM_QUAD : G1_FFT_FORM_LANE; }
// the form of the stage with the most ladders of `count` transforms of length 2^logn (the last stage of a pass: every
// stage of a call takes its own decision, this is the one the tests aim at)
inline int g1_fft_form_at(int logn, uint64_t count, uint64_t quad_max) {
    return g1_fft_form(count * g1_fft_ladders(logn, logn), quad_max);
}

// The chunks of a batch of n blobs on one device: chunk c covers [c * chunk, min(n, (c + 1) * chunk)).
inline uint64_t domain_chunk_count(uint64_t n, uint64_t chunk) { return chunk ? (n + chunk - 1) / chunk : 0; }
inline uint64_t domain_chunk_size(uint64_t n, uint64_t chunk, uint64_t c) {
    const uint64_t lo = c * chunk;
    if (lo >= n) return 0;
    return n - lo < chunk ? n - lo : chunk;
}

// ---- the openings (ckzg_hip_compute_coset_kzg_proofs_batch, ckzg_hip_compute_domain_kzg_proofs_batch) ----
// Coset size l = 2^e, e <= COSET_MAX_LOG; k = 4096 / l rows; l Toeplitz columns of length 2k = 8192 / l, which fill one
// row of 8192 column-major: slot t of a row is position t mod 2k of column t / 2k.  m = 2k proofs per blob on the
// cosets; the domain call is e = 0 and keeps the 4096 proofs of the evaluation domain.
constexpr int COSET_MAX_LOG = 6;
HD uint32_t coset_proofs_per_blob(int e) { return 8192u >> e; }

// Column i of the circulant (toeplitz_coeffs_stride(p, i, l), src/eip7594/fk20.c): v_i[0] = p[4095 - i],
// v_i[1 .. k+1] = 0, v_i[k+2+j] = p[2l - i - 1 + j l].  Returns the coefficient index that slot t of the row reads, or
// -1 for a zero slot.  N = 4096 in the product; the tests also run smaller N.  At e = 0 (one column of length 2N):
// v[0] = p[N-1], v[1 .. N+1] = 0, v[N+2+j] = p[1+j] for j = 0 .. N-3.
HD int coset_circulant_source(uint32_t t, int e, uint32_t N) {
    const uint32_t l = 1u << e, k = N >> e, i = t / (2u * k), pos = t - i * 2u * k;
    if (pos == 0) return (int)(N - 1u - i);
    if (pos >= k + 2u) return (int)(2u * l - i - 1u + (pos - k - 2u) * l);
    return -1;
}

// The setup vector of column i before its transform: X_i[j] = g1_values_monomial[N - l - 1 - i - j l] for j < k - 1,
// the identity above (setup.c:238-330).  Returns the monomial index that slot t of the row reads, or -1 for the identity.
// At e = 0: N - 2 - t for t <= N - 2.
HD int coset_setup_source(uint32_t t, int e, uint32_t N) {
    const uint32_t l = 1u << e, k = N >> e, i = t / (2u * k), j = t - i * 2u * k;
    if (j + 1u >= k) return -1;
    return (int)(N - l - 1u - i - j * l);
}

// The column sum u[t] = sum_{i < l} product[i][t] runs as strided passes, one lane per output and pass, the lanes of a
// wave on consecutive t.  One pass of l sequential additions leaves 8192 / l lanes per blob, so above
// COSET_COLSUM_RADIX columns the sum is split: `parts` lanes per output each add the columns i = part (mod parts) into
// row `part` (COSET_COLSUM_RADIX additions deep), then one lane adds the `parts` rows.  parts == 1: a single pass.
constexpr uint32_t COSET_COLSUM_RADIX = 8;
HD uint32_t coset_colsum_parts(int e) { return (1u << e) > COSET_COLSUM_RADIX ? (1u << e) / COSET_COLSUM_RADIX : 1u; }

}  // namespace ckzg
