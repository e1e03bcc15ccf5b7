// weight_pack.h -- the host side of every weight layout the kernels read: plain C++ into std::vector, no HIP calls.
// One GEMM view of the weights (GemmWeights), one fp32 fragment packer and one 16-bit piece packer; a layout is the small
// callable that says which (row, channel, tap) lane `lane` holds in element `e` of step `st`.
// Self-contained: any host compiler with _Float16 (clang, gcc 13) compiles it on its own.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/parrot_hip.h"

namespace parrot {

// what the host needs to know of a split scheme (PARROT_PREC_* = the ID of the kernels' Sch* struct, conv_split.h)
inline int scheme_pieces(int scheme) { return scheme == PARROT_PREC_BF16X6 ? 3 : scheme == PARROT_PREC_F16X3 ? 2 : 1; }
inline bool scheme_is_f16(int scheme) { return scheme == PARROT_PREC_F16X3 || scheme == PARROT_PREC_F16; }
inline float scheme_xs(int scheme) { return scheme_is_f16(scheme) ? 8.f : 1.f; }

inline uint16_t f16_rn_host(float x) {  // round-to-nearest-even, overflow -> inf (what v_cvt_pk_f16_f32 does)
    const _Float16 h = (_Float16)x;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
inline float f16_to_f(uint16_t u) {
    _Float16 h;
    memcpy(&h, &u, 2);
    return (float)h;
}
inline uint16_t bf16_rn_host(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_to_f(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// Split-scheme weight pieces (conv_split.h).  fp16 schemes: the layer's weights are scaled by the power of two that puts
// max|w| into [2^14, 2^15), so the second piece of every weight that matters is a normal fp16 number.
inline float f16_weight_scale(const float* w, size_t n) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(w[i]));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.f;
    int e;
    (void)std::frexp(mx, &e);  // mx = m * 2^e, m in [0.5, 1)
    return std::ldexp(1.f, 15 - e);  // mx * scale in [2^14, 2^15)
}
inline void split_weight(float v, int scheme, float wscale, uint16_t (&h)[3]) {
    h[0] = h[1] = h[2] = 0;
    if (scheme_is_f16(scheme)) {
        const float vs = v * wscale;
        h[0] = f16_rn_host(vs);
        if (scheme == PARROT_PREC_F16X3) h[1] = f16_rn_host(vs - f16_to_f(h[0]));
        return;
    }
    h[0] = bf16_rn_host(v);
    if (scheme == PARROT_PREC_BF16X6) {
        const float r1 = v - bf16_to_f(h[0]);
        h[1] = bf16_rn_host(r1);
        h[2] = bf16_rn_host(r1 - bf16_to_f(h[1]));
    }
}

// W'(m, i, j) of the GEMM view of a conv: row m, input channel i (of the row's group), tap j; 0 outside the real extents.
//   plain / grouped conv, torch layout (c_out, c_in / groups, k): W' = w[m][i][j];
//   transposed conv, torch layout (c_in, c_out, k), in polyphase gather form: row m = o * u + r (output channel o, phase r) reads
//   tap kappa = r + padding - (j + dmin) * u of input t + j + dmin.
struct GemmWeights {
    const float* w;
    int M, Cin, k;       // GEMM rows, input channels per group, taps of the torch weight
    bool transposed;
    int c_out, u, padding, dmin;  // (transposed only)
    float operator()(int m, int i, int j) const {
        if (m >= M || i >= Cin) return 0.f;
        if (transposed) {
            const int o = m / u, r = m % u;
            const int kap = r + padding - (j + dmin) * u;
            return (kap >= 0 && kap < k) ? w[((size_t)i * c_out + o) * k + kap] : 0.f;
        }
        // (j >= k: the 16-channel ResBlock stream packs taps in pairs, and the second tap of the last pair of an odd k does not exist)
        return j < k ? w[((size_t)m * Cin + i) * k + j] : 0.f;
    }
};
struct WeightAt {
    int m, i, j;
};

// The exact-fp32 conv adds all c_in * k products of an output along ONE accumulator, an MFMA (2 products) per rounding.  At n_fft =
// 1024 that chain took the f32 log-mel past 4 x d_ref on white noise; a spec that is exact before its rounding to fp32 leaves 0.25 x
// (DESIGN.md section 4).  So the PARROT_PREC_F32 plans of the mel handle (DFT) and the aligner run as GROUPED convs: group g sums the
// g-th G-th of the input channels into its own `rows` rows (padded to whole 128-row tiles: Mg) and a following kernel adds the G
// partials.  G: the largest count <= 8 that leaves whole 16-channel slabs per group; a c_in that is no multiple of 32 keeps one chain.
struct ChainGroups { int G, Mg; };
inline ChainGroups chain_groups(int scheme, int cin, int rows) {
    int G = 1;
    if (scheme == PARROT_PREC_F32)
        for (int g = 8; g > 1 && G == 1; --g)
            if (cin % (16 * g) == 0) G = g;
    return {G, G > 1 ? (rows + 127) / 128 * 128 : rows};
}

// fp32 MFMA fragments: n_steps groups of [lane][4] floats at dst, element (lane, e) of step st = W'(at(st, lane, e))
template <typename Layout>
inline void pack_f32(float* dst, size_t n_steps, const GemmWeights& W, Layout at) {
    for (size_t st = 0; st < n_steps; ++st)
        for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 4; ++e) {
                const WeightAt q = at(st, lane, e);
                dst[st * 256 + lane * 4 + e] = W(q.m, q.i, q.j);
            }
}
// 16-bit MFMA operands of a split scheme: n_steps steps of [piece][lane][8 x 16 bit] at dst
template <typename Layout>
inline void pack_pieces(uint16_t* dst, size_t n_steps, int scheme, float wscale, const GemmWeights& W, Layout at) {
    const int NP = scheme_pieces(scheme);
    for (size_t st = 0; st < n_steps; ++st) {
        uint16_t* g = dst + st * NP * 512;
        for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 8; ++e) {
                const WeightAt q = at(st, lane, e);
                uint16_t h[3];
                split_weight(W(q.m, q.i, q.j), scheme, wscale, h);
                for (int pc = 0; pc < NP; ++pc) g[pc * 512 + lane * 8 + e] = h[pc];
            }
    }
}

}  // namespace parrot
