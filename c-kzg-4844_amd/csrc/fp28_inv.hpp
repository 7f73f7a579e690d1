// fp28_inv.hpp -- modular inversion in Fp by the Bernstein-Yang "safegcd" divstep iteration
// (variable-time form; nothing here is secret).  A Fermat ladder costs 381 dependent squarings
// (~2*10^5 instructions per lane); 30 divsteps at a time on the low words of (f, g), followed by
// one 2x2-matrix update of the full-width (f, g) and of the cofactors (d, e), costs ~600
// instructions per batch and at most ~40 batches.
//
//   divstep(eta, f, g):  g odd and eta < 0 -> (-eta - 1, g, (g - f)/2)
//                        g odd             -> ( eta - 1, f, (g + f)/2)
//                        g even            -> ( eta - 1, f,  g/2)
// Invariant: f = d*x, g = e*x (mod p) for the input x; when g reaches 0, f = +-1 and d = +-1/x.
// Limbs: 13 signed words of 30 bits; 64-bit signed accumulators (v_mad_i64_i32).  d and e are kept
// exactly divisible by 2^30 at every update by adding a multiple of p, so no power of two is left
// over; each update lets |d|, |e| grow by at most p, which 13 x 30 bits absorb for the <= 40
// batches the iteration can take (768 divsteps suffice for 381-bit inputs; 40*30 = 1200).
//
// The update step and the driver loop are written once, for a modulus given as a parameter struct: Fp here, Fr on
// 9 limbs in fr_inv.hpp (fr_inv_safegcd) and fr29.hpp (fr29_inv).  Each of the three keeps only its own repacking
// into and out of 30-bit limbs and its own final Montgomery product.
#pragma once
#include "fp28.hpp"

namespace ckzg {

struct DivstepMatrix {
    int32_t u, v, q, r;
};

// A limb stored as (int32_t)(c & M) is, to the compiler, still the 64-bit value it was cut from, and its next product
// with a matrix entry becomes a 64 x 64-bit multiplication (v_mad_u64_u32 + two v_mul_lo_u32 + a v_add3_u32 of sign
// corrections).  Passing the limb through an empty asm makes it a plain 32-bit register again, and
// (int64_t)a * b is ONE v_mad_i64_i32: 661 -> ~230 instructions per update of (f, g) and (d, e).
HD int32_t limb32(int32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#endif
    return x;
}

// 30 divsteps on the low 30 bits of f and g; returns the new eta.
// Variable-time form (nothing here is secret): a run of zero bits of g is ONE step (count trailing zeros, shift g and
// the matrix column by the run), and an odd g has its bottom min(eta + 1, bits left, 6) bits cancelled at once by the
// multiple w = -g/f mod 2^6 of f -- for odd f, f (f^2 - 2) = -1/f mod 64 -- which is what that many consecutive
// divsteps would add up to.  A batch of 30 divsteps is ~6 trips round this loop instead of 30 round the bit-by-bit
// one: the inversion that closes every commitment, every proof batch and every step of the table builder drops from
// ~31,000 to ~13,000 instructions of one lane.
HD int32_t divsteps30(int32_t eta, uint32_t f, uint32_t g, DivstepMatrix &t) {
    uint32_t u = 1, v = 0, q = 0, r = 1;
    int left = 30;
    for (;;) {
        // zeros of g, counted only up to the bits that are left (sentinel above them)
        const uint32_t sentinel = g | (0xffffffffu << left);
#if defined(__HIP_DEVICE_COMPILE__)
        const int zeros = (int)__builtin_ctz(sentinel);
#else
        const int zeros = __builtin_ctz(sentinel);
#endif
        g >>= zeros;
        u <<= zeros;
        v <<= zeros;
        eta -= zeros;
        left -= zeros;
        if (left == 0) break;
        // g is odd
        if (eta < 0) {
            eta = -eta;
            uint32_t tmp = f;
            f = g;
            g = 0u - tmp;
            tmp = u;
            u = q;
            q = 0u - tmp;
            tmp = v;
            v = r;
            r = 0u - tmp;
        }
        // no more bits than are left, and no more than eta + 1 (after that many the sign of eta flips)
        int limit = eta + 1 > left ? left : eta + 1;
        if (limit > 6) limit = 6;
        const uint32_t m = (1u << limit) - 1u;
        const uint32_t w = (g * f * (f * f - 2u)) & m;   // -g/f mod 2^limit
        g += f * w;
        q += u * w;
        r += v * w;
    }
    t.u = limb32((int32_t)u);
    t.v = limb32((int32_t)v);
    t.q = limb32((int32_t)q);
    t.r = limb32((int32_t)r);
    return eta;
}

// What the iteration needs of a modulus m on N signed 30-bit limbs: its limbs, 1/m mod 2^30, a multiple K m above the
// bound on |d| (|d| grows by at most m per batch) and the number of batches that always suffices.
struct Safegcd30Fp {   // p: 768 divsteps suffice for 381-bit inputs; |d| < 41 p, and 13 x 30 bits hold it
    static constexpr int N = 13, MAXIT = 40;
    static constexpr uint32_t MINV = FP30_PINV;
    HD static constexpr int32_t mod(int i) { return FP30_P[i]; }
    HD static constexpr int32_t kmod(int i) { return FP30_64P[i]; }
};
struct Safegcd30Fr {   // r: 738 divsteps suffice for 255-bit inputs; |d| < 27 r, and 9 x 30 bits hold 2^14 r
    static constexpr int N = 9, MAXIT = 26;
    static constexpr uint32_t MINV = FR30_RINV;
    HD static constexpr int32_t mod(int i) { return FR30_R[i]; }
    HD static constexpr int32_t kmod(int i) { return FR30_32R[i]; }
};

// (f, g) <- t * (f, g) / 2^30, exact
template <class P>
HD void update_fg30(int32_t *f, int32_t *g, const DivstepMatrix &t) {
    constexpr int N = P::N;
    const int64_t M = (1 << 30) - 1;
    int64_t cf = (int64_t)t.u * f[0] + (int64_t)t.v * g[0];
    int64_t cg = (int64_t)t.q * f[0] + (int64_t)t.r * g[0];
    cf >>= 30;
    cg >>= 30;
#pragma unroll
    for (int i = 1; i < N; i++) {
        cf += (int64_t)t.u * f[i] + (int64_t)t.v * g[i];
        cg += (int64_t)t.q * f[i] + (int64_t)t.r * g[i];
        f[i - 1] = limb32((int32_t)(cf & M));
        g[i - 1] = limb32((int32_t)(cg & M));
        cf >>= 30;
        cg >>= 30;
    }
    f[N - 1] = limb32((int32_t)cf);
    g[N - 1] = limb32((int32_t)cg);
}

// (d, e) <- t * (d, e) / 2^30 mod m: a multiple of m makes the low 30 bits vanish first
template <class P>
HD void update_de30(int32_t *d, int32_t *e, const DivstepMatrix &t) {
    const int64_t M = (1 << 30) - 1;
    int64_t cd = (int64_t)t.u * d[0] + (int64_t)t.v * e[0];
    int64_t ce = (int64_t)t.q * d[0] + (int64_t)t.r * e[0];
    const int32_t md = (int32_t)(((0u - (uint32_t)cd) * P::MINV) & (uint32_t)M);
    const int32_t me = (int32_t)(((0u - (uint32_t)ce) * P::MINV) & (uint32_t)M);
    cd += (int64_t)P::mod(0) * md;
    ce += (int64_t)P::mod(0) * me;
    cd >>= 30;
    ce >>= 30;
#pragma unroll
    for (int i = 1; i < P::N; i++) {
        cd += (int64_t)t.u * d[i] + (int64_t)t.v * e[i] + (int64_t)P::mod(i) * md;
        ce += (int64_t)t.q * d[i] + (int64_t)t.r * e[i] + (int64_t)P::mod(i) * me;
        d[i - 1] = limb32((int32_t)(cd & M));
        e[i - 1] = limb32((int32_t)(ce & M));
        cd >>= 30;
        ce >>= 30;
    }
    d[P::N - 1] = limb32((int32_t)cd);
    e[P::N - 1] = limb32((int32_t)ce);
}

// The iteration itself: g = x != 0 (mod m) as 30-bit limbs (clobbered); w = 1/x mod m as a positive integer, in 30-bit
// words with the top one holding what is left.  Batches of 30 divsteps until g = 0; then f = +1 or -1 and the result is
// f * d, made positive by adding K m.  |d| < (MAXIT + 1) m, so w < K m + (MAXIT + 1) m: 105 p for p, 59 r for r.
template <class P>
HD void safegcd30(uint32_t *w, int32_t *g) {
    constexpr int N = P::N;
    int32_t f[N], d[N], e[N];
    for (int i = 0; i < N; i++) {
        f[i] = P::mod(i);
        d[i] = 0;
        e[i] = 0;
    }
    e[0] = 1;
    int32_t eta = -1;
    for (int it = 0; it < P::MAXIT; it++) {
        DivstepMatrix t;
        eta = divsteps30(eta, (uint32_t)f[0], (uint32_t)g[0], t);
        update_de30<P>(d, e, t);
        update_fg30<P>(f, g, t);
        int32_t nz = 0;
        for (int i = 0; i < N; i++) nz |= g[i];
        if (nz == 0) break;
    }
    const bool negate = f[N - 1] < 0;
    int64_t c = 0;
    for (int i = 0; i < N; i++) {
        c += (int64_t)P::kmod(i) + (negate ? -(int64_t)d[i] : (int64_t)d[i]);
        w[i] = (uint32_t)(c & 0x3fffffff);
        c >>= 30;
    }
    w[N - 1] += (uint32_t)(c << 30);
}

// 1/a in the 2^392 Montgomery domain; 0 for a == 0 (mod p), like the Fermat ladder
HDNI inline F28<1, 2> f28_inv_safegcd(const F28<1, 2> &a) {
    if (is_zero(a)) {
        F28<1, 2> z;
        for (int j = 0; j < 14; j++) z.l[j] = 0;
        return z;
    }
    int32_t g[13];
    // 14 x 28-bit limbs (value < 2p < 2^382) -> 13 x 30-bit limbs
    for (int i = 0; i < 13; i++) {
        int bit = 30 * i, j = bit / 28, sh = bit - 28 * j;
        uint32_t v = a.l[j] >> sh;
        if (j + 1 < 14) v |= a.l[j + 1] << (28 - sh);
        if (28 - sh + 28 < 30 && j + 2 < 14) v |= a.l[j + 2] << (56 - sh);
        g[i] = (int32_t)(v & 0x3fffffffu);
    }
    uint32_t w[13];   // below 105p < 2^388
    safegcd30<Safegcd30Fp>(w, g);
    // 13 x 30 -> 14 x 28
    F28<1, 128> y;
    for (int j = 0; j < 14; j++) {
        int bit = 28 * j, i = bit / 30, sh = bit - 30 * i;
        uint32_t v = w[i] >> sh;
        if (i + 1 < 13 && 30 - sh < 28) v |= w[i + 1] << (30 - sh);
        y.l[j] = (j == 13) ? v : (v & M28);
    }
    // y = 1/(a R) as an integer; Montgomery-multiply by R^3 to land on (1/a) R
    return mul(y, f28_const<1, 1>(FP28_R3));
}

}  // namespace ckzg
