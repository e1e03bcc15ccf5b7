// host_gan_loss.hip -- the vocoder's adversarial losses (feature_loss, generator_loss, discriminator_loss) with their gradients:
// validation, the workspace layout and the launches of gan_loss.h.  Stateless: no handle, no device allocation, no copy, no
// host synchronisation.
#include "host_common.h"

#include <algorithm>

#include "gan_loss.h"

using namespace parrot;

// n <= 2^36 per term: a launch's 64 terms then hold fewer than 2^31 tiles
static constexpr int64_t GAN_MAX_N = (int64_t)1 << 36;
static int64_t gan_tiles(int64_t n) { return (n + GAN_TILE - 1) / GAN_TILE; }

// the one layout: a tile sum per tile of the whole table, then a mean per term
static size_t gan_ws(Arena& a, int64_t tiles, int32_t K, double** part, double** mean) {
    *part = a.take<double>((size_t)tiles);
    *mean = a.take<double>((size_t)K);
    return align_up(a.off, 256);
}

extern "C" int32_t parrot_gan_loss_tile(void) { return GAN_TILE; }

extern "C" size_t parrot_gan_loss_workspace_bytes(const parrot_gan_term_t* terms, int32_t K) {
    if (!terms || K <= 0) return 0;
    int64_t tiles = 0;
    for (int32_t k = 0; k < K; ++k) {
        if (terms[k].n < 0 || terms[k].n > GAN_MAX_N) return 0;
        tiles += gan_tiles(terms[k].n);
    }
    Arena a(nullptr, 0);
    double *part, *mean;
    return gan_ws(a, tiles, K, &part, &mean);
}

extern "C" int parrot_gan_loss(const parrot_gan_term_t* terms, int32_t K, const double* weights, double scale, double* term_out, float* total,
                               void* ws, size_t ws_bytes, void* stream) {
    if (K < 0 || (K > 0 && !terms)) return fail(PARROT_E_INVALID, "gan_loss: null term table or negative K");
    const bool values = term_out || total;
    bool any_grad = false;
    int64_t tiles = 0;
    for (int32_t k = 0; k < K; ++k) {
        const parrot_gan_term_t& t = terms[k];
        const std::string who = "gan_loss: term " + std::to_string(k);
        if (t.op != PARROT_GAN_L1 && t.op != PARROT_GAN_SQ1 && t.op != PARROT_GAN_SQ0) return fail(PARROT_E_INVALID, who + ": unknown op " + std::to_string(t.op));
        if (t.n < 0) return fail(PARROT_E_INVALID, who + ": negative n");
        if (t.n > GAN_MAX_N) return fail(PARROT_E_UNSUPPORTED, who + ": more than 2^36 elements");
        if (!t.a) return fail(PARROT_E_INVALID, who + ": null a");
        if (t.op == PARROT_GAN_L1 && !t.b) return fail(PARROT_E_INVALID, who + ": null b (PARROT_GAN_L1 takes two arrays)");
        if (t.op != PARROT_GAN_L1 && t.grad_b) return fail(PARROT_E_INVALID, who + ": grad_b on a squares term (b is unused)");
        for (const float* g : {(const float*)t.grad_a, (const float*)t.grad_b})
            if (g && (g == t.a || (t.op == PARROT_GAN_L1 && g == t.b))) return fail(PARROT_E_INVALID, who + ": a gradient must not alias its input");
        any_grad = any_grad || t.grad_a || t.grad_b;
        tiles += gan_tiles(t.n);
    }
    if (!values && !any_grad) return fail(PARROT_E_INVALID, "gan_loss: neither values (term_out / total) nor a gradient requested");
    double *part = nullptr, *mean = nullptr;
    if (values && K > 0) {  // (a backward alone takes no workspace)
        if (!ws) return fail(PARROT_E_INVALID, "gan_loss: null workspace");
        Arena a(ws, ws_bytes);
        (void)gan_ws(a, tiles, K, &part, &mean);
        if (!a.ok) return fail(PARROT_E_NOMEM, "gan_loss: workspace too small");
    }
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(term_out, (size_t)K * sizeof(double), s));
        TRY(poison(total, sizeof(float), s));
        for (int32_t k = 0; k < K; ++k) {
            TRY(poison(terms[k].grad_a, (size_t)terms[k].n * sizeof(float), s));
            TRY(poison(terms[k].grad_b, (size_t)terms[k].n * sizeof(float), s));
        }
    }
    // PARROT_GAN_MAX_TERMS terms per launch; the last launch's reduction also forms the total over every term
    int32_t k0 = 0;
    do {
        GanLaunch L{};
        L.K = std::min<int32_t>(K - k0, PARROT_GAN_MAX_TERMS);
        for (int32_t k = 0; k < L.K; ++k) {
            L.t[k] = terms[k0 + k];
            L.tile0[k + 1] = L.tile0[k] + (int32_t)gan_tiles(L.t[k].n);
        }
        const bool last = k0 + L.K >= K;
        if (L.K > 0) HIP_TRY(launch_gan_tiles(L, weights ? weights + k0 : nullptr, part, values, s));
        if (values)
            HIP_TRY(launch_gan_reduce(L, part, mean ? mean + k0 : nullptr, term_out ? term_out + k0 : nullptr, mean, K, scale, last ? total : nullptr, s));
        if (part) part += L.tile0[L.K];
        k0 += L.K;
    } while (k0 < K);
    return PARROT_OK;
}
