// host_mel.hip -- the log-mel handle and the mel L1 (kernels in mel.h).
#include "host_common.h"

#include <cmath>
#include <vector>

#include "mel.h"
#include "weight_pack.h"

using namespace parrot;

// ---------------------------------------------------------------------------------------------
// Log-mel spectrogram + mel L1 (reference utils/vocoder/dataset.py:43-69, utils/vocoder/train.py:213): kernels in mel.h, the two
// GEMMs -- framed DFT, mel projection -- as parrot_conv plans owned by the handle.
// ---------------------------------------------------------------------------------------------
struct parrot_mel {
    parrot_mel_cfg cfg{};
    int F = 0, Fp = 0, k = 0, pad_r = 0;  // n_fft / 2 + 1 bins (padded to 16 for the mel conv), taps, reflect pad
    int G = 1, Mg = 0;                    // channel groups of the framed DFT and spec rows per group (mel_create)
    int scheme = PARROT_PREC_F16X3;
    std::unique_ptr<parrot_conv> stft, proj;
    // the adjoints of the two (parrot_mel_l1_grad): n_mels padded to 16-channel chunks; 2F padded to MEL_BWD_GROUPS whole groups
    // of 16-channel chunks; rows per group of the transposed DFT (hop padded to whole 128-row tiles)
    int Mp = 0, C2p = 0, Mgt = 0;
    std::unique_ptr<parrot_conv> proj_t, stft_t;
    DevFlag err;
};

static int mel_create(parrot_mel_t** out, const parrot_mel_cfg* cfg, const float* window, const float* basis, int prec) {
    if (!out || !cfg || !window || !basis) return fail(PARROT_E_INVALID, "mel_create: null argument");
    const int n_fft = cfg->n_fft, hop = cfg->hop, win = cfg->win, n_mels = cfg->n_mels;
    if (n_fft < 2 || hop < 1 || hop > n_fft || win < 1 || win > n_fft || n_mels < 1) return fail(PARROT_E_INVALID, "mel_create: need 1 <= hop <= n_fft, 1 <= win <= n_fft, n_mels >= 1");
    int scheme;  // the metric does not move with the vocoder's operating point: the single-MFMA modes are not offered here
    TRY(resolve_parity_prec(prec, "mel_create", &scheme));
    CreateScope scope(scheme, -1, -1);
    query_device();
    std::unique_ptr<parrot_mel> m(new parrot_mel());
    m->cfg = *cfg;
    m->scheme = scheme;
    m->F = n_fft / 2 + 1;
    m->Fp = (m->F + 15) / 16 * 16;
    m->k = (n_fft + hop - 1) / hop;
    m->pad_r = (n_fft - hop) / 2;
    const int F = m->F, k = m->k;
    // W[o][c][j] = w[n] cos(2 pi f n / n_fft) (rows [0, F)), -w[n] sin(...) (rows [F, 2F)), n = j hop + c, zero for n >= n_fft; w = the
    // fp32 window zero-padded, centred, to n_fft as torch.stft does; formed in fp64 with the angle reduced as (f n) mod n_fft
    std::vector<double> wpad((size_t)n_fft, 0.0);
    const int left = (n_fft - win) / 2;
    for (int i = 0; i < win; ++i) wpad[(size_t)left + i] = (double)window[i];
    // PARROT_PREC_F32: a GROUPED conv (chain_groups, weight_pack.h; hop 256: 8 groups of 32 channels, hop 160: 5 of 32), summed by the magnitude kernel
    const ChainGroups cgr = chain_groups(scheme, hop, 2 * F);
    const int G = cgr.G, Mg = cgr.Mg, cg = hop / G;
    m->G = G;
    m->Mg = Mg;
    std::vector<float> W((size_t)G * Mg * cg * k, 0.f);  // (G Mg, hop / G, k): torch's grouped layout
    // ... and its adjoint from the same fp64-formed values: Wt[c][o][j'] = W[o][c][k - 1 - j'] -- with padding k - 1 that conv is
    // g_poly[c][tau] = sum_o sum_j W[o][c][j] g_spec[o][tau - j].  It sums 2F k products per output: like the forward's f32 DFT it
    // runs as a GROUPED conv, group g adding the g-th MEL_BWD_GROUPS-th of the spec rows into its own Mgt rows (torch's grouped
    // layout (G Mgt, C2p / G, k)); mel_frame_adjoint_kernel adds the partials.
    m->Mp = (n_mels + 15) / 16 * 16;
    m->C2p = (2 * F + 16 * MEL_BWD_GROUPS - 1) / (16 * MEL_BWD_GROUPS) * (16 * MEL_BWD_GROUPS);
    m->Mgt = (hop + 127) / 128 * 128;
    const int cgt = m->C2p / MEL_BWD_GROUPS, Mgt = m->Mgt;
    std::vector<float> Wt((size_t)MEL_BWD_GROUPS * Mgt * cgt * k, 0.f);
    auto wt_at = [&](int c, int o, int j) -> float& { return Wt[(((size_t)(o / cgt) * Mgt + c) * cgt + o % cgt) * k + j]; };
    const double two_pi = 6.283185307179586476925286766559;
    for (int f = 0; f < F; ++f)
        for (int c = 0; c < hop; ++c)
            for (int j = 0; j < k; ++j) {
                const int n = j * hop + c;
                if (n >= n_fft) continue;
                const double ang = two_pi * (double)(((long long)f * n) % n_fft) / (double)n_fft;
                const size_t row = (size_t)(c / cg) * Mg + f;
                W[(row * cg + c % cg) * k + j] = (float)(wpad[n] * std::cos(ang));
                W[((row + F) * cg + c % cg) * k + j] = (float)(-wpad[n] * std::sin(ang));
                wt_at(c, f, k - 1 - j) = (float)(wpad[n] * std::cos(ang));
                wt_at(c, F + f, k - 1 - j) = (float)(-wpad[n] * std::sin(ang));
            }
    TRY(make_conv(m->stft, hop, G * Mg, k, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, W.data(), nullptr, G));
    std::vector<float> P((size_t)n_mels * m->Fp, 0.f);
    for (int o = 0; o < n_mels; ++o)
        for (int f = 0; f < F; ++f) P[(size_t)o * m->Fp + f] = basis[(size_t)o * F + f];
    TRY(make_conv(m->proj, m->Fp, n_mels, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, P.data(), nullptr));
    {   // The transposed plans run in exact fp32 (conv_mfma_kernel) under EVERY handle precision: 1 / mel reaches 5e4, beyond what
        // fp16x3 holds (8190), and the split schemes add each of their 3 / 6 piece products into the fp32 accumulator on its own,
        // several roundings per 16-channel step, which the gradient's allowance (2 x torch's fp32 error) does not leave room for
        // over 2F k products (measured: DESIGN.md section 4).  The DFT's adjoint is grouped as above; basis^T sums n_mels products
        // and stays one chain.  The exact-fp32 handle's G forward partials are summed by mel_magnitude_bwd_kernel: its adjoint
        // takes the same single (B, C2p, T) operand as the others'.
        CreateScope bwd(PARROT_PREC_F32, -1, -1);
        std::vector<float> Pt((size_t)m->Fp * m->Mp, 0.f);
        for (int o = 0; o < n_mels; ++o)
            for (int f = 0; f < F; ++f) Pt[(size_t)f * m->Mp + o] = basis[(size_t)o * F + f];
        TRY(make_conv(m->proj_t, m->Mp, m->Fp, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, Pt.data(), nullptr));
        TRY(make_conv(m->stft_t, m->C2p, MEL_BWD_GROUPS * Mgt, k, 1, k - 1, 0, 1, PRE_NONE, 0.f, ACT_NONE, Wt.data(), nullptr, MEL_BWD_GROUPS));
    }
    TRY(m->err.init());
    *out = m.release();
    return PARROT_OK;
}
extern "C" int parrot_mel_create(parrot_mel_t** out, const parrot_mel_cfg* cfg, const float* window_host, const float* basis_host) {
    return mel_create(out, cfg, window_host, basis_host, -1);
}
extern "C" int parrot_mel_create_ex(parrot_mel_t** out, const parrot_mel_cfg* cfg, const float* window_host, const float* basis_host,
                                    int32_t precision) {
    return mel_create(out, cfg, window_host, basis_host, precision);
}
extern "C" void parrot_mel_destroy(parrot_mel_t* m) { delete m; }
extern "C" int parrot_mel_precision(const parrot_mel_t* m) { return m ? m->scheme : PARROT_E_INVALID; }
extern "C" int parrot_mel_frames(const parrot_mel_t* m, int32_t n_samples) { return (m && n_samples >= 0) ? n_samples / m->cfg.hop : PARROT_E_INVALID; }

struct MelScratch {
    float *poly, *spec, *mag;
};
static MelScratch mel_scratch(const parrot_mel* m, Arena& a, int B, int N) {
    const size_t T = (size_t)(N / m->cfg.hop);
    MelScratch w{};
    w.poly = a.take<float>((size_t)B * m->cfg.hop * (T + m->k - 1));
    w.spec = a.take<float>((size_t)B * m->G * m->Mg * T);
    w.mag = a.take<float>((size_t)B * m->Fp * T);
    return w;
}
extern "C" size_t parrot_mel_workspace_bytes(const parrot_mel_t* m, int32_t B, int32_t N) {
    if (!m || B <= 0 || N < m->cfg.hop) return 0;
    Arena a(nullptr, 0);
    (void)mel_scratch(m, a, B, N);
    return align_up(a.off, 256);
}
// the forward up to the pre-log mel (B, n_mels, T)
static int mel_forward_pre(parrot_mel* m, const float* wav, int64_t row_stride, const int32_t* n_samples, int B, int N, const MelScratch& w,
                           float* mel_pre, hipStream_t s) {
    const int hop = m->cfg.hop, T = N / hop, Tc = T + m->k - 1;
    hipLaunchKernelGGL(mel_frame_kernel, dim3((Tc + 63) / 64, (hop + 63) / 64, B), dim3(256), 0, s, wav, (long)row_stride, n_samples, N, hop, m->k,
                       m->pad_r, Tc, w.poly, m->err);
    HIP_TRY(hipGetLastError());
    TRY(conv_launch(m->stft.get(), w.poly, nullptr, w.spec, B, Tc, EPI_STORE, 1.f, s));
    const size_t n_mag = (size_t)B * m->Fp * T;
    if (T % 4 == 0 && (((uintptr_t)w.spec | (uintptr_t)w.mag) & 15) == 0)
        hipLaunchKernelGGL(mel_magnitude_kernel<4>, dim3((unsigned)((n_mag / 4 + 255) / 256)), dim3(256), 0, s, w.spec, w.mag, m->F, m->Fp, T, m->G, m->Mg,
                           n_mag / 4);
    else
        hipLaunchKernelGGL(mel_magnitude_kernel<1>, dim3((unsigned)((n_mag + 255) / 256)), dim3(256), 0, s, w.spec, w.mag, m->F, m->Fp, T, m->G, m->Mg, n_mag);
    HIP_TRY(hipGetLastError());
    return conv_launch(m->proj.get(), w.mag, nullptr, mel_pre, B, T, EPI_STORE, 1.f, s);
}
extern "C" int parrot_mel_forward(parrot_mel_t* m, const float* wav, int64_t row_stride, const int32_t* n_samples, int32_t B, int32_t N,
                                  float* mel_out, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !wav || !mel_out || !ws) return fail(PARROT_E_INVALID, "mel_forward: null argument");
    const int hop = m->cfg.hop, n_mels = m->cfg.n_mels;
    if (B <= 0 || B > 65535 || N < hop || row_stride < N) return fail(PARROT_E_INVALID, "mel_forward: need 1 <= B <= 65535, N >= hop (one frame) and row_stride >= N");
    hipStream_t s = (hipStream_t)stream;
    const int T = N / hop;
    Arena a(ws, ws_bytes);
    const MelScratch w = mel_scratch(m, a, B, N);
    if (!a.ok) return fail(PARROT_E_NOMEM, "mel_forward: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(mel_out, (size_t)B * n_mels * T * sizeof(float), s));
    }
    TRY(mel_forward_pre(m, wav, row_stride, n_samples, B, N, w, mel_out, s));
    const size_t n_out = (size_t)B * n_mels * T;
    hipLaunchKernelGGL(mel_log_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, mel_out, n_samples, N, hop, n_mels, T, n_out, m->err);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}

static int mel_l1_blocks(int n_mels, int T) { return (int)(((long)n_mels * T + MEL_L1_CHUNK - 1) / MEL_L1_CHUNK); }
extern "C" size_t parrot_mel_l1_workspace_bytes(int32_t B, int32_t n_mels, int32_t T) {
    if (B <= 0 || n_mels <= 0 || T <= 0) return 0;
    return align_up((size_t)B * mel_l1_blocks(n_mels, T) * sizeof(double), 256);
}
extern "C" int parrot_mel_l1(const float* a, const float* b, const int32_t* n_frames, int32_t B, int32_t n_mels, int32_t T, double* out_f64,
                             float* mean_f32, void* ws, size_t ws_bytes, void* stream) {
    if (!a || !b || !out_f64 || !ws) return fail(PARROT_E_INVALID, "mel_l1: null argument");
    if (B <= 0 || B > 65535 || n_mels <= 0 || T <= 0) return fail(PARROT_E_INVALID, "mel_l1: need 1 <= B <= 65535 and non-empty spectrograms");
    if (ws_bytes < parrot_mel_l1_workspace_bytes(B, n_mels, T)) return fail(PARROT_E_NOMEM, "mel_l1: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(out_f64, (size_t)2 * B * sizeof(double), s));
        TRY(poison(mean_f32, sizeof(float), s));
    }
    const int nblk = mel_l1_blocks(n_mels, T);
    hipLaunchKernelGGL(mel_l1_rows_kernel, dim3(nblk, B), dim3(256), 0, s, a, b, n_frames, n_mels, T, (double*)ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mel_l1_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, n_frames, B, n_mels, T, out_f64, mean_f32);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// Loss + gradient with respect to the waveform: the forward, the L1 pair, five stages backwards (mel.h).
// ---------------------------------------------------------------------------------------------
struct MelGradScratch {
    MelScratch fwd;
    float *mel, *logmel, *g_mel, *g_mag, *g_spec, *g_poly, *factor;
    double* part;
    int32_t* n_frames;
};
static MelGradScratch mel_grad_scratch(const parrot_mel* m, Arena& a, int B, int N) {
    const size_t T = (size_t)(N / m->cfg.hop), n_mels = (size_t)m->cfg.n_mels;
    MelGradScratch w{};
    w.fwd = mel_scratch(m, a, B, N);
    w.mel = a.take<float>(B * n_mels * T);
    w.logmel = a.take<float>(B * n_mels * T);
    w.g_mel = a.take<float>((size_t)B * m->Mp * T);
    w.g_mag = a.take<float>((size_t)B * m->Fp * T);
    w.g_spec = a.take<float>((size_t)B * m->C2p * T);
    w.g_poly = a.take<float>((size_t)B * MEL_BWD_GROUPS * m->Mgt * (T + m->k - 1));
    w.part = a.take<double>((size_t)B * mel_l1_blocks((int)n_mels, (int)T));
    w.n_frames = a.take<int32_t>((size_t)B);
    w.factor = a.take<float>(1);
    return w;
}
extern "C" size_t parrot_mel_l1_grad_workspace_bytes(const parrot_mel_t* m, int32_t B, int32_t N) {
    if (!m || B <= 0 || N < m->cfg.hop) return 0;
    Arena a(nullptr, 0);
    (void)mel_grad_scratch(m, a, B, N);
    return align_up(a.off, 256);
}
extern "C" int parrot_mel_l1_grad(parrot_mel_t* m, const float* wav, int64_t row_stride, const int32_t* n_samples, const float* target, int32_t B,
                                  int32_t N, int32_t reduction, double scale, double* out_f64, void* loss, float* grad_wav, void* ws,
                                  size_t ws_bytes, void* stream) {
    if (!m || !wav || !target || !out_f64 || !loss || !grad_wav || !ws) return fail(PARROT_E_INVALID, "mel_l1_grad: null argument");
    const int hop = m->cfg.hop, n_mels = m->cfg.n_mels;
    if (B <= 0 || B > 65535 || N < hop || row_stride < N) return fail(PARROT_E_INVALID, "mel_l1_grad: need 1 <= B <= 65535, N >= hop (one frame) and row_stride >= N");
    if (reduction != PARROT_MEL_REDUCE_MEAN && reduction != PARROT_MEL_REDUCE_SUM) return fail(PARROT_E_INVALID, "mel_l1_grad: reduction is PARROT_MEL_REDUCE_MEAN or PARROT_MEL_REDUCE_SUM");
    hipStream_t s = (hipStream_t)stream;
    const bool mean = reduction == PARROT_MEL_REDUCE_MEAN;
    const int T = N / hop, Tc = T + m->k - 1;
    Arena a(ws, ws_bytes);
    const MelGradScratch w = mel_grad_scratch(m, a, B, N);
    if (!a.ok) return fail(PARROT_E_NOMEM, "mel_l1_grad: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(out_f64, (size_t)2 * B * sizeof(double), s));
        TRY(poison(loss, mean ? sizeof(float) : sizeof(double), s));
        TRY(poison(grad_wav, (size_t)B * N * sizeof(float), s));
    }
    // forward, with the pre-log mel kept
    TRY(mel_forward_pre(m, wav, row_stride, n_samples, B, N, w.fwd, w.mel, s));
    const size_t n_out = (size_t)B * n_mels * T;
    hipLaunchKernelGGL(mel_log_keep_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, w.mel, w.logmel, n_samples, N, hop, n_mels, T, n_out, m->err);
    HIP_TRY(hipGetLastError());
    // the loss: parrot_mel_l1's kernels on (logmel, target, n_samples / hop)
    const int32_t* nf = nullptr;
    if (n_samples) {
        hipLaunchKernelGGL(mel_frames_kernel, dim3((B + 255) / 256), dim3(256), 0, s, n_samples, N, hop, B, w.n_frames);
        HIP_TRY(hipGetLastError());
        nf = w.n_frames;
    }
    const int nblk = mel_l1_blocks(n_mels, T);
    hipLaunchKernelGGL(mel_l1_rows_kernel, dim3(nblk, B), dim3(256), 0, s, w.logmel, target, nf, n_mels, T, w.part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mel_l1_reduce_kernel, dim3(1), dim3(256), 0, s, w.part, nblk, nf, B, n_mels, T, out_f64, mean ? (float*)loss : nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mel_l1_scale_kernel, dim3(1), dim3(256), 0, s, out_f64, B, mean ? 1 : 0, scale, w.factor, mean ? nullptr : (double*)loss);
    HIP_TRY(hipGetLastError());
    // backwards: head -> basis^T -> magnitude -> DFT^T -> frame adjoint
    const size_t n_gmel = (size_t)B * m->Mp * T, n_gspec = (size_t)B * m->C2p * T;
    hipLaunchKernelGGL(mel_l1_head_kernel, dim3((unsigned)((n_gmel + 255) / 256)), dim3(256), 0, s, w.mel, w.logmel, target, n_samples, N, hop, n_mels, m->Mp, T,
                       n_gmel, w.g_mel);
    HIP_TRY(hipGetLastError());
    TRY(conv_launch(m->proj_t.get(), w.g_mel, nullptr, w.g_mag, B, T, EPI_STORE, 1.f, s));
    hipLaunchKernelGGL(mel_magnitude_bwd_kernel, dim3((unsigned)((n_gspec + 255) / 256)), dim3(256), 0, s, w.fwd.spec, w.fwd.mag, w.g_mag, m->F, m->Fp, m->C2p, T,
                       m->G, m->Mg, n_gspec, w.g_spec);
    HIP_TRY(hipGetLastError());
    TRY(conv_launch(m->stft_t.get(), w.g_spec, nullptr, w.g_poly, B, T, EPI_STORE, 1.f, s));
    const int n_cols = (int)(((long)N + m->pad_r - 1) / hop + 1);
    hipLaunchKernelGGL(mel_frame_adjoint_kernel, dim3((n_cols + 63) / 64, (hop + 63) / 64, B), dim3(256), 0, s, w.g_poly, n_samples, N, hop, m->k, m->cfg.n_fft,
                       m->pad_r, Tc, MEL_BWD_GROUPS, m->Mgt, w.factor, grad_wav, m->err);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}

static int mel_status(int h) {
    if (h == MEL_ST_SHORT_ROW)
        return fail(PARROT_E_INVALID, "mel: a row is no longer than the reflect pad (n_fft - hop) / 2 (torch: Padding size should be less than the corresponding input dimension)");
    return fail(PARROT_E_NONFINITE, "mel: non-finite mel or gradient value (a NaN / inf input sample, or a magnitude beyond the fp16 split scheme's range: use PARROT_PREC_BF16X6 or PARROT_PREC_F32)");
}
extern "C" int parrot_mel_check(parrot_mel_t* m, void* stream) { return m ? check_flag(m->err, (hipStream_t)stream, mel_status) : PARROT_E_INVALID; }
extern "C" int parrot_mel_status_async(parrot_mel_t* m, int32_t* dst_dev, void* stream) { return m ? status_async(m->err, dst_dev, (hipStream_t)stream) : PARROT_E_INVALID; }
