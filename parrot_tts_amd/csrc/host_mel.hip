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
            }
    TRY(make_conv(m->stft, hop, G * Mg, k, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, W.data(), nullptr, G));
    std::vector<float> P((size_t)n_mels * m->Fp, 0.f);
    for (int o = 0; o < n_mels; ++o)
        for (int f = 0; f < F; ++f) P[(size_t)o * m->Fp + f] = basis[(size_t)o * F + f];
    TRY(make_conv(m->proj, m->Fp, n_mels, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, P.data(), nullptr));
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
extern "C" int parrot_mel_forward(parrot_mel_t* m, const float* wav, int64_t row_stride, const int32_t* n_samples, int32_t B, int32_t N,
                                  float* mel_out, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !wav || !mel_out || !ws) return fail(PARROT_E_INVALID, "mel_forward: null argument");
    const int hop = m->cfg.hop, n_mels = m->cfg.n_mels;
    if (B <= 0 || B > 65535 || N < hop || row_stride < N) return fail(PARROT_E_INVALID, "mel_forward: need 1 <= B <= 65535, N >= hop (one frame) and row_stride >= N");
    hipStream_t s = (hipStream_t)stream;
    const int T = N / hop, Tc = T + m->k - 1;
    Arena a(ws, ws_bytes);
    const MelScratch w = mel_scratch(m, a, B, N);
    if (!a.ok) return fail(PARROT_E_NOMEM, "mel_forward: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(mel_out, (size_t)B * n_mels * T * sizeof(float), s));
    }
    hipLaunchKernelGGL(mel_frame_kernel, dim3((Tc + 63) / 64, (hop + 63) / 64, B), dim3(256), 0, s, wav, (long)row_stride, n_samples, N, hop, m->k,
                       m->pad_r, Tc, w.poly, m->err);
    HIP_TRY(hipGetLastError());
    TRY(conv_launch(m->stft.get(), w.poly, nullptr, w.spec, B, Tc, EPI_STORE, 1.f, s));
    const size_t n_mag = (size_t)B * m->Fp * T, n_out = (size_t)B * n_mels * T;
    if (T % 4 == 0 && (((uintptr_t)w.spec | (uintptr_t)w.mag) & 15) == 0)
        hipLaunchKernelGGL(mel_magnitude_kernel<4>, dim3((unsigned)((n_mag / 4 + 255) / 256)), dim3(256), 0, s, w.spec, w.mag, m->F, m->Fp, T, m->G, m->Mg,
                           n_mag / 4);
    else
        hipLaunchKernelGGL(mel_magnitude_kernel<1>, dim3((unsigned)((n_mag + 255) / 256)), dim3(256), 0, s, w.spec, w.mag, m->F, m->Fp, T, m->G, m->Mg, n_mag);
    HIP_TRY(hipGetLastError());
    TRY(conv_launch(m->proj.get(), w.mag, nullptr, mel_out, B, T, EPI_STORE, 1.f, s));
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

static int mel_status(int h) {
    if (h == MEL_ST_SHORT_ROW)
        return fail(PARROT_E_INVALID, "mel: a row is no longer than the reflect pad (n_fft - hop) / 2 (torch: Padding size should be less than the corresponding input dimension)");
    return fail(PARROT_E_NONFINITE, "mel: non-finite mel value (a NaN / inf input sample, or a magnitude beyond the fp16 split scheme's range: use PARROT_PREC_BF16X6 or PARROT_PREC_F32)");
}
extern "C" int parrot_mel_check(parrot_mel_t* m, void* stream) { return m ? check_flag(m->err, (hipStream_t)stream, mel_status) : PARROT_E_INVALID; }
extern "C" int parrot_mel_status_async(parrot_mel_t* m, int32_t* dst_dev, void* stream) { return m ? status_async(m->err, dst_dev, (hipStream_t)stream) : PARROT_E_INVALID; }
