// div_uniform.h -- x / d for a divisor that is the same for every element of a launch (the MRF branch mean: d = number of
// ResBlock branches, 3 for every shipped config), bit for bit the IEEE quotient without the 10-instruction division sequence
// (v_div_scale x2, v_rcp, v_fma x4, v_div_fmas, v_div_fixup) per element:
//   DIV_MUL   d a power of two whose reciprocal is a normal number: x * (1 / d), ONE rounding of the same real number as x / d
//   DIV_FMA3  d == 3:  q = x r;  e = fma(-q, d, x);  q' = fma(e, r, q)  with r = RN(1 / 3)   -- the residual e is exact, the
//             correction rounds once.  Two classes of x need the select, which keeps q wherever e is zero or NaN (one
//             v_cmp_lg_f32): x = +-inf gives e = NaN (inf - inf) and x = -0 gives e = +0, hence q' = +0, where q is already
//             the quotient (an e of zero changes no other q; a NaN x gives a NaN q either way).
//             tools/probes/div3_exhaustive.cpp compares all 2^32 inputs with x / 3.
//   DIV_TRUE  anything else: the division.
// Host and device compile the same text (the exhaustive check runs it with the host compiler).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PARROT_HD __host__ __device__ __forceinline__
#else
#define PARROT_HD inline
#endif

namespace parrot {

enum { DIV_TRUE = 0, DIV_MUL = 1, DIV_FMA3 = 2 };

struct DivUniform {
    float d, r;  // divisor; RN(1 / d) (exact in DIV_MUL)
    int mode;
};

PARROT_HD DivUniform div_uniform(float d) {
    DivUniform u;
    u.d = d;
    u.r = 1.f / d;
    uint32_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
    bits = __builtin_bit_cast(uint32_t, d);
#else
    std::memcpy(&bits, &d, 4);
#endif
    const uint32_t ex = (bits >> 23) & 0xff;  // 2^(ex - 127); the reciprocal 2^(127 - ex) is normal for ex <= 253
    const bool pow2 = (bits & 0x007fffffu) == 0 && ex >= 1 && ex <= 253;
    u.mode = pow2 ? DIV_MUL : (d == 3.f ? DIV_FMA3 : DIV_TRUE);
    return u;
}

PARROT_HD float div3_fma(float x, float d, float r) {
    const float q = x * r;
    const float e = __builtin_fmaf(-q, d, x);
    return (e < 0.f || e > 0.f) ? __builtin_fmaf(e, r, q) : q;
}

// one element; the MFMA kernels use div_rows so that the mode is tested once per group of registers
PARROT_HD float div_apply(const DivUniform& u, float x) {
    if (u.mode == DIV_FMA3) return div3_fma(x, u.d, u.r);
    if (u.mode == DIV_MUL) return x * u.r;
    return x / u.d;
}

template <int N>
PARROT_HD void div_rows(const DivUniform& u, float (&v)[N]) {
    if (u.mode == DIV_FMA3) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = div3_fma(v[i], u.d, u.r);
    } else if (u.mode == DIV_MUL) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = v[i] * u.r;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = v[i] / u.d;
    }
}

}  // namespace parrot
