// gn_dropout.h -- the attention-dropout mask (training mode): a pure, counter-based function of
// (key, layer, internal edge id, head), stated in include/gotennet_hip.h.  One Philox4x32-10 evaluation per element,
// output word 0; nothing is stored between the forward (which applies it in the softmax kernels' final write) and the
// backward (which reads the two attention arrays and draws nothing).
#pragma once
#include "gn_common.h"

namespace gn {

// Philox4x32-10 (Salmon et al., SC'11; Random123): the four output words of counter (c0..c3) under key (k0, k1)
__device__ __forceinline__ uint4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const unsigned hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return make_uint4(c0, c1, c2, c3);
}
// output word 0 alone (the dropout mask)
__device__ __forceinline__ unsigned philox4x32_10_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                                        unsigned k0, unsigned k1) {
    return philox4x32_10(c0, c1, c2, c3, k0, k1).x;
}

struct AttnDrop {
    float* a_soft;              // [E,H] the undropped weights (softmax * norm)
    const long long* key;       // device: {seed, reserved}
    unsigned layer, thresh;     // keep iff word >= thresh = floor(p 2^32)
    float scale;                // 1 / (1 - p), rounded once to fp32
    int all;                    // p >= 1: everything is dropped
};

// multiplier of element n = e * H + h: 0 or 1 / (1 - p)
__device__ __forceinline__ float drop_mult(unsigned k0, unsigned k1, unsigned layer, unsigned thresh, float scale, int all,
                                           unsigned long long n) {
    if (all) return 0.f;
    const unsigned w = philox4x32_10_word0((unsigned)n, (unsigned)(n >> 32), layer, 0u, k0, k1);
    return w >= thresh ? scale : 0.f;
}

}  // namespace gn
