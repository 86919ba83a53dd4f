// The LoRA dropout mask: a pure function of (seed, row, column, stream, step), the same on the device, in host C++ and in numpy (llava_mi355x/dropout.py).
//
// What it stands for: peft gives every adapted linear its own nn.Dropout, y = base(x) + scaling * lora_B(lora_A(dropout(x))), and the reference's LoRA scripts run
// it at p = 0.05 (llava/train/train.py:113, :879).  Here nothing is stashed: the forward, a recomputed layer and the two backward kernels regenerate the bits.
//
//   generator   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's philox4x32_10)
//   one call    per aligned group of 8 columns (the 16-byte chunk of a 16-bit row): counter = (row, col >> 3, stream, step), key = the 64-bit seed (lo, hi)
//   keep rule   the four output words are eight 16-bit lanes; column c takes word (c & 7) >> 1, low half for even c; keep iff lane >= thr = round(p * 65536):
//               the drop probability is p rounded to a multiple of 2^-16
//   value       kept: T(x * fp32(1 / (1 - p))), ONE rounding to the tensor's dtype (peft's dropout output is a tensor of that dtype); dropped: +0
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LMX_HD __host__ __device__
#else
#define LMX_HD
#endif

namespace lmx {

struct DropSpec {
    uint32_t seed_lo, seed_hi, step, stream, thr;
    float scale;
};

LMX_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// thr and the fp32 scale of a drop probability 0 <= p < 1 (checked by the callers)
inline uint32_t dropout_thr(double p) { return (uint32_t)(int64_t)(p * 65536.0 + 0.5); }
inline float dropout_scale(double p) { return (float)(1.0 / (1.0 - p)); }
inline DropSpec make_drop_spec(double p, uint64_t seed, uint32_t step, uint32_t stream) {
    return DropSpec{(uint32_t)seed, (uint32_t)(seed >> 32), step, stream, dropout_thr(p), dropout_scale(p)};
}

// bit j: column 8 * col8 + j of row `row` is kept
LMX_HD inline uint32_t dropout_keep8(const DropSpec& d, uint32_t row, uint32_t col8) {
    uint32_t w[4];
    philox4x32_10(row, col8, d.stream, d.step, d.seed_lo, d.seed_hi, w);
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m |= ((w[i] & 0xffffu) >= d.thr ? 1u : 0u) << (2 * i);
        m |= ((w[i] >> 16) >= d.thr ? 1u : 0u) << (2 * i + 1);
    }
    return m;
}

}  // namespace lmx
