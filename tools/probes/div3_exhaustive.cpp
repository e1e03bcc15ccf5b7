// Exhaustive host check of csrc/div_uniform.h: for each divisor on the command line (default 3) every one of the 2^32 fp32
// bit patterns x -- subnormals, infinities, NaNs -- goes through div_apply and is compared with x / d bit for bit (two NaNs count
// as equal).  `--stride S` as the first argument visits every S-th pattern only.  One JSON line per divisor, with the path
// div_uniform chose for it; exit status 1 on any mismatch.  Seconds per divisor on 16 threads.
//   g++ -O2 -std=c++17 -ffp-contract=off -pthread tools/probes/div3_exhaustive.cpp -o build_exp/div3_exhaustive && build_exp/div3_exhaustive
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../parrot_tts_amd/csrc/div_uniform.h"

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static uint32_t to_bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

int main(int argc, char** argv) {
    std::vector<float> ds;
    unsigned long long stride = 1;
    int first = 1;
    if (argc > 2 && std::strcmp(argv[1], "--stride") == 0) {
        stride = std::strtoull(argv[2], nullptr, 10);
        first = 3;
    }
    if (stride == 0) return 2;
    for (int i = first; i < argc; ++i) ds.push_back(std::strtof(argv[i], nullptr));
    if (ds.empty()) ds = {3.f};
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = hw == 0 ? 4 : (hw > 16 ? 16 : (int)hw);
    bool all_ok = true;
    for (const float d : ds) {
        volatile float dv = d;  // (the reference division must not be folded into a multiply by the compiler)
        const parrot::DivUniform u = parrot::div_uniform(d);
        std::atomic<unsigned long long> bad{0}, first_bad{~0ull};
        std::vector<std::thread> th;
        const unsigned long long total = 1ull << 32, per = total / nthreads;
        for (int t = 0; t < nthreads; ++t) {
            const unsigned long long lo = t * per, hi = (t + 1 == nthreads) ? total : lo + per;
            th.emplace_back([&, lo, hi]() {
                const float dd = dv;
                unsigned long long nbad = 0, fb = ~0ull;
                for (unsigned long long i = (lo + stride - 1) / stride * stride; i < hi; i += stride) {
                    const float x = from_bits((uint32_t)i);
                    const float want = x / dd, got = parrot::div_apply(u, x);
                    const bool same = (want != want) ? (got != got) : to_bits(want) == to_bits(got);
                    if (!same) {
                        ++nbad;
                        if (fb == ~0ull) fb = i;
                    }
                }
                bad += nbad;
                unsigned long long cur = first_bad.load();
                while (fb < cur && !first_bad.compare_exchange_weak(cur, fb)) {}
            });
        }
        for (auto& t : th) t.join();
        const char* mode = u.mode == parrot::DIV_FMA3 ? "fma3" : u.mode == parrot::DIV_MUL ? "mul" : "true";
        std::printf("{\"probe\": \"div_exhaustive\", \"d\": %g, \"mode\": \"%s\", \"r_bits\": \"0x%08x\", \"inputs\": %llu, \"mismatches\": %llu, \"first_mismatch_bits\": ",
                    (double)d, mode, to_bits(u.r), (total + stride - 1) / stride, bad.load());
        if (bad.load()) std::printf("\"0x%08llx\"}\n", first_bad.load());
        else std::printf("null}\n");
        all_ok = all_ok && bad.load() == 0;
    }
    return all_ok ? 0 : 1;
}
