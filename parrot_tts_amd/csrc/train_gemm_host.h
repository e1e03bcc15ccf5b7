// train_gemm_host.h -- host only: the products of the training units (host_aligner_train.hip, host_tte_train.hip,
// host_voc_train.hip; host_mpd_train.hip fills the structs itself for its strided convs; host_msd_train.hip uses conv_fwd / _dx / _dw for its one dense conv) as launches of train_gemm.h.  An activation array is described by three strides, a weight by torch's own
// layout, and conv forward, data gradient and weight gradient are written once over the two; a Linear is the k = 1 conv over all its
// rows as one batch row.  Every function returns PARROT_OK or what fail() returned.
#pragma once
#include <algorithm>

#include "host_common.h"
#include "train_gemm.h"

namespace parrot {

// Where an activation array keeps element (b, c, t): at b sz + c sc + t st.
struct Lay {
    long sz, sc, st;
};
inline Lay chan_first(int C, int T) { return Lay{(long)C * T, T, 1}; }     // (B, C, T)
inline Lay chan_last(int T, long ld) { return Lay{(long)T * ld, 1, ld}; }  // (B, T, ld): channel c of frame t at column c of a row of ld
// A conv weight as torch holds it, (cout, cin, k); tap j reads the input at t + j dil - pad.  A Linear (out, in): k = 1, pad = 0.
struct ConvW {
    const float* w;
    int cout, cin, k, dil, pad;
};
// What tap_gemm_kernel's epilogue adds to the product, in the kernel's order (pre, the last field, comes before the mask); all zero: nothing
struct Epi {
    const float *bias0 = nullptr, *bias1 = nullptr;
    const float* mask = nullptr;
    float mslope = 0.f;
    const float* res = nullptr;
    int relu = 0, lrelu = 0;
    float lslope = 0.f;
    const float* pre = nullptr;
};
inline void set_epi(TapGemmParams& g, const Epi& e) {
    g.bias0 = e.bias0; g.bias1 = e.bias1; g.mask = e.mask; g.mslope = e.mslope; g.res = e.res; g.relu = e.relu; g.lrelu = e.lrelu; g.lslope = e.lslope; g.pre = e.pre;
}

// Y[b][co][t] = epi(sum_j sum_ci W[co][ci][j] X[b][ci][t + j dil - pad])
inline int conv_fwd(const ConvW& w, const float* X, Lay lx, float* Y, Lay ly, int B, int T, const Epi& e, hipStream_t s) {
    TapGemmParams g{};
    g.ntaps = w.k;
    for (int j = 0; j < w.k; ++j) { g.A[j] = w.w + j; g.shift[j] = j * w.dil - w.pad; }
    g.a_sm = (long)w.cin * w.k; g.a_sk = w.k;
    g.X = X; g.x_sz = lx.sz; g.x_sk = lx.sc; g.x_sn = lx.st;
    g.C = Y; g.c_sz = ly.sz; g.c_sm = ly.sc; g.c_sn = ly.st;
    g.M = w.cout; g.N = T; g.K = w.cin;
    set_epi(g, e);
    HIP_TRY(launch_tap_gemm(g, B, s));
    return PARROT_OK;
}
// dX[b][ci][t] = epi(sum_j sum_co W[co][ci][j] dY[b][co][t - (j dil - pad)]): the same launch with W transposed through its strides
// and the shifts negated
inline int conv_dx(const ConvW& w, const float* dY, Lay ly, float* dX, Lay lx, int B, int T, const Epi& e, hipStream_t s) {
    TapGemmParams g{};
    g.ntaps = w.k;
    for (int j = 0; j < w.k; ++j) { g.A[j] = w.w + j; g.shift[j] = w.pad - j * w.dil; }
    g.a_sm = w.k; g.a_sk = (long)w.cin * w.k;
    g.X = dY; g.x_sz = ly.sz; g.x_sk = ly.sc; g.x_sn = ly.st;
    g.C = dX; g.c_sz = lx.sz; g.c_sm = lx.sc; g.c_sn = lx.st;
    g.M = w.cin; g.N = T; g.K = w.cout;
    set_epi(g, e);
    HIP_TRY(launch_tap_gemm(g, B, s));
    return PARROT_OK;
}

// The weight-gradient partials (chunks x taps x M x K floats, chunks = ceil(B T / 256)) are formed for as many taps at a time as fit
// in WG_BUDGET bytes, and always for at least one: a layer's buffer is at most max(64 MiB, chunks x one tap's M x K x 4 bytes).
constexpr size_t WG_BUDGET = (size_t)64 << 20;
// floats of partial buffer for a layer of k taps of mk = M K elements each over R = B T pairs
inline size_t wgrad_part_floats(int R, size_t mk, int k) {
    const size_t chunks = (size_t)wgrad_chunks(R);
    return chunks * std::max(mk, std::min(mk * k, WG_BUDGET / sizeof(float) / chunks));
}
// taps per launch: what fits the buffer and wgrad_kernel's grid.z = chunks x taps
inline int wgrad_group(int k, int chunks, size_t mk, size_t part_floats) {
    const int G = (int)std::min<size_t>((size_t)k, part_floats / ((size_t)chunks * mk));
    return std::max(1, std::min(G, 65535 / chunks));
}
// q (ntaps, shift and part aside) for taps of shifts[0 .. k), a group at a time: the partials, then their fp64 sum in chunk order
// into out[m o_sm + kk o_sk + j o_sj]
inline int wgrad_taps(WgradParams q, const int* shifts, int k, float* out, long o_sm, long o_sk, long o_sj, float* part, size_t part_floats,
                      hipStream_t s) {
    const int chunks = wgrad_chunks(q.R), G = wgrad_group(k, chunks, (size_t)q.M * q.K, part_floats);
    q.part = part;
    for (int j0 = 0; j0 < k; j0 += G) {
        q.ntaps = std::min(G, k - j0);
        for (int j = 0; j < q.ntaps; ++j) q.shift[j] = shifts[j0 + j];
        HIP_TRY(launch_wgrad(q, s));
        HIP_TRY(launch_wgrad_reduce(part, chunks, q.ntaps, q.M, q.K, out + j0 * o_sj, o_sm, o_sk, o_sj, s));
    }
    return PARROT_OK;
}
// dW[co][ci][j] = sum_(b, t) dY[b][co][t] X[b][ci][t + j dil - pad], in torch's layout (w.w is not read)
inline int conv_dw(const ConvW& w, const float* dY, Lay ly, const float* X, Lay lx, float* dW, int B, int T, float* part, size_t part_floats,
                   hipStream_t s) {
    WgradParams q{};
    q.dY = dY; q.y_sz = ly.sz; q.y_sm = ly.sc; q.y_st = ly.st;
    q.X = X; q.x_sz = lx.sz; q.x_sk = lx.sc; q.x_st = lx.st;
    q.M = w.cout; q.K = w.cin; q.T = T; q.R = B * T;
    int shifts[TG_MAX_TAPS];
    for (int j = 0; j < w.k; ++j) shifts[j] = j * w.dil - w.pad;
    return wgrad_taps(q, shifts, w.k, dW, (long)w.cin * w.k, w.k, 1, part, part_floats, s);
}
// out0[m] (and out1[m], nullable) = the sum of column m over the rows of src (rows, M; row stride ld); part: chunks x M doubles
inline int colsum(const float* src, long rows, int M, long ld, double* part, float* out0, float* out1, hipStream_t s) {
    HIP_TRY(launch_colsum(src, (int)rows, M, ld, part, out0, out1, s));
    return PARROT_OK;
}

}  // namespace parrot
