// naf2.hpp -- the plain NAF recoding of the pipelined twiddle ladders (g1_pipe.hpp), in a header of its own because
// it is compiled for host and device while the pipeline is device only (host_shim.cpp tests the host form).
#pragma once
#include "field.hpp"

namespace ckzg {
namespace quad {

constexpr int NAF2_LEN = 130;     // plain NAF of a value < 2^129

// Plain (width-2) non-adjacent form of a 128-bit k: digits in {0, +-1}, no two adjacent non-zero, density 1/3.
HDNI inline void naf2_128(int8_t *out, const uint32_t *k) {
    uint32_t v[5] = {k[0], k[1], k[2], k[3], 0};
    for (int i = 0; i < NAF2_LEN; i++) {
        int d = 0;
        if (v[0] & 1u) {
            d = 2 - (int)(v[0] & 3u);   // 1 -> +1, 3 -> -1
            if (d > 0) {
                v[0] &= ~1u;            // v -= 1 (v is odd)
            } else {
                uint64_t c = 1;         // v += 1
                for (int j = 0; j < 5 && c; j++) {
                    uint64_t t = (uint64_t)v[j] + c;
                    v[j] = (uint32_t)t;
                    c = t >> 32;
                }
            }
        }
        out[i] = (int8_t)d;
        for (int j = 0; j < 4; j++) v[j] = (v[j] >> 1) | (v[j + 1] << 31);
        v[4] >>= 1;
    }
}

}  // namespace quad
}  // namespace ckzg
