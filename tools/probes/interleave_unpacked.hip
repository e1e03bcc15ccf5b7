// Which VALU instruction classes collide with the matrix pipe on gfx950, and which hide in the gaps an MFMA leaves in a SIMD's
// vector issue?  interleave.hip measured ONE filler mix (the operand conversion's, a quarter of it packed fp32) and found
// "MFMA + n VALU = M + V".  This sibling takes the mix apart.  Fillers, n = 2 / 4 / 6 per MFMA, all volatile inline asm (the issue
// order is the source order), on registers the MFMAs do not touch, random operands everywhere:
//     mix            today's write_p mix: v_pk_mul_f32 x2, v_max_f32 x2, v_cvt_pk_f16_f32, v_fma_mix_f32 x2, v_cvt_pk_f16_f32 (cyclic)
//     mix_unpacked   the same with each v_pk_mul_f32 replaced by two v_mul_f32 (10 instructions for the same work as the 8 above)
//     one class on its own: v_mul_f32, v_pk_mul_f32, v_max_f32, v_cvt_pk_f16_f32, v_fma_mix_f32, v_permlane32_swap, ds_write_b128
// for v_mfma_f32_32x32x16_f16 and v_mfma_f32_16x16x32_f16, in three placements (one wave per SIMD = 4 per workgroup, or two):
//     same_wave      every wave issues the MFMA and its n fillers
//     other_wave     waves 0-3 issue MFMAs only, waves 4-7 (the same four SIMDs) issue n fillers per MFMA slot only
//     filler_alone   waves 4-7 as above, waves 0-3 idle: what the fillers cost with the matrix pipe empty (V)
// and the MFMA stream alone (filler "none": M).  Each wave times its own loop with s_memtime, which counts shader clocks here (the
// MFMA stream alone reads 32.4 / 17.2 per MFMA at the boost clock and at the power-limited clock of 256 busy CUs alike, while the
// wall time per MFMA goes from 13.7 to 20.6 ns); `clk_per_mfma_slot` is the slower role's clocks per MFMA (slot), so serialised
// issue reads M + V and hidden issue max(M, V).  `ns_kernel_per_slot` is the launch's wall time (HIP events) over the slots.
//   hipcc --offload-arch=gfx950 -O3 tools/probes/interleave_unpacked.hip -o build_exp/interleave_unpacked
//   build_exp/interleave_unpacked > profiles/rNN_interleave_unpacked.jsonl
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <utility>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

enum { F_MIX = 0, F_MIX_UNPACKED, F_MUL, F_PK_MUL, F_MAX, F_CVT, F_FMA_MIX, F_PERMLANE, F_DS_WRITE, F_COUNT };
static const char* const FILL_NAME[F_COUNT] = {"mix", "mix_unpacked", "v_mul_f32", "v_pk_mul_f32", "v_max_f32", "v_cvt_pk_f16_f32",
                                               "v_fma_mix_f32", "v_permlane32_swap", "ds_write_b128"};
enum { P_SAME = 0, P_OTHER = 1, P_ALONE = 2 };
static const char* const PLACE_NAME[3] = {"same_wave", "other_wave", "filler_alone"};

struct Regs {  // two independent register groups [q] so that consecutive instructions of one kind do not chain
    f32x2 a[2], b[2], k2;
    float s0[2], s1[2], t0[2], t1[2], k;
    float x0[2], x1[2], m0[2], m1[2], r0[2], r1[2];
    unsigned h[2], l[2], pa[2], pb[2];
    u32x4 ld;
    unsigned laddr;
};
#define MUL(d, s) asm volatile("v_mul_f32 %0, %1, %2" : "=v"(d) : "v"(s), "v"(R.k))
#define PKMUL(d, s) asm volatile("v_pk_mul_f32 %0, %1, %2" : "=v"(d) : "v"(s), "v"(R.k2))
#define MAXF(d, x, y) asm volatile("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(y))
#define CVT(d, x, y) asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(y))
#define MIXLO(d, hh, x) asm volatile("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hh), "v"(x))
#define MIXHI(d, hh, x) asm volatile("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hh), "v"(x))
template <int FILL, int I>
__device__ __forceinline__ void fill_one(Regs& R) {
    if constexpr (FILL == F_MIX) {
        constexpr int s = I % 8, q = (I / 8) % 2;
        if constexpr (s == 0) PKMUL(R.b[q], R.a[q]);
        else if constexpr (s == 1) PKMUL(R.a[q], R.b[q]);
        else if constexpr (s == 2) MAXF(R.m0[q], R.x0[q], R.x1[q]);
        else if constexpr (s == 3) MAXF(R.m1[q], R.x1[q], R.x0[q]);
        else if constexpr (s == 4) CVT(R.h[q], R.m0[q], R.m1[q]);
        else if constexpr (s == 5) MIXLO(R.r0[q], R.h[q], R.m0[q]);
        else if constexpr (s == 6) MIXHI(R.r1[q], R.h[q], R.m1[q]);
        else CVT(R.l[q], R.r0[q], R.r1[q]);
    } else if constexpr (FILL == F_MIX_UNPACKED) {
        constexpr int s = I % 10, q = (I / 10) % 2;
        if constexpr (s == 0) MUL(R.t0[q], R.s0[q]);
        else if constexpr (s == 1) MUL(R.t1[q], R.s1[q]);
        else if constexpr (s == 2) MUL(R.s0[q], R.t0[q]);
        else if constexpr (s == 3) MUL(R.s1[q], R.t1[q]);
        else if constexpr (s == 4) MAXF(R.m0[q], R.x0[q], R.x1[q]);
        else if constexpr (s == 5) MAXF(R.m1[q], R.x1[q], R.x0[q]);
        else if constexpr (s == 6) CVT(R.h[q], R.m0[q], R.m1[q]);
        else if constexpr (s == 7) MIXLO(R.r0[q], R.h[q], R.m0[q]);
        else if constexpr (s == 8) MIXHI(R.r1[q], R.h[q], R.m1[q]);
        else CVT(R.l[q], R.r0[q], R.r1[q]);
    } else {
        constexpr int q = I % 2, back = (I / 2) % 2;
        if constexpr (FILL == F_MUL) {
            if constexpr (back) MUL(R.s0[q], R.t0[q]);
            else MUL(R.t0[q], R.s0[q]);
        } else if constexpr (FILL == F_PK_MUL) {
            if constexpr (back) PKMUL(R.a[q], R.b[q]);
            else PKMUL(R.b[q], R.a[q]);
        } else if constexpr (FILL == F_MAX) {
            if constexpr (back) MAXF(R.m1[q], R.x1[q], R.x0[q]);
            else MAXF(R.m0[q], R.x0[q], R.x1[q]);
        } else if constexpr (FILL == F_CVT) {
            if constexpr (back) CVT(R.l[q], R.x1[q], R.x0[q]);
            else CVT(R.h[q], R.x0[q], R.x1[q]);
        } else if constexpr (FILL == F_FMA_MIX) {
            if constexpr (back) MIXHI(R.r1[q], R.h[q], R.x1[q]);
            else MIXLO(R.r0[q], R.h[q], R.x0[q]);
        } else if constexpr (FILL == F_PERMLANE) {
            asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(R.pa[q]), "+v"(R.pb[q]));
        } else {
            asm volatile("ds_write_b128 %0, %1" ::"v"(R.laddr), "v"(R.ld));
        }
    }
}
template <int FILL, int BASE, int N>
__device__ __forceinline__ void fill_n(Regs& R) {
    if constexpr (N > 0) {
        fill_one<FILL, BASE>(R);
        fill_n<FILL, BASE + 1, N - 1>(R);
    }
}

// SHAPE 0: 16x16x32 (4 accumulators of f32x4), 1: 32x32x16 (2 accumulators of f32x16).  SLOTS MFMA slots per loop iteration: 20, so
// that SLOTS * NV fillers are whole cycles of both mixes (8 and 10 instructions) for NV = 2, 4, 6.
constexpr int SLOTS = 20;
template <int SHAPE, int FILL, int NV, bool DO_M, bool DO_V, int G>
__device__ __forceinline__ void slot(Regs& R, f32x4 (&c4)[4], f32x16 (&c16)[2], const f16x8& a, const f16x8& b) {
    if constexpr (G < SLOTS) {
        if constexpr (DO_M) {
            if constexpr (SHAPE == 0) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c4[G & 3]) : "v"(a), "v"(b));
            else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(c16[G & 1]) : "v"(a), "v"(b));
        }
        if constexpr (DO_V) fill_n<FILL, G * NV, NV>(R);
        slot<SHAPE, FILL, NV, DO_M, DO_V, G + 1>(R, c4, c16, a, b);
    }
}
template <int SHAPE, int FILL, int NV, bool DO_M, bool DO_V>
__device__ __forceinline__ void slots(Regs& R, f32x4 (&c4)[4], f32x16 (&c16)[2], const f16x8& a, const f16x8& b, int iters) {
    for (int it = 0; it < iters; ++it) {
        slot<SHAPE, FILL, NV, DO_M, DO_V, 0>(R, c4, c16, a, b);
        if constexpr (DO_V && FILL == F_DS_WRITE) asm volatile("s_waitcnt lgkmcnt(0)");
    }
}

template <int SHAPE, int FILL, int NV, int PLACE>
__global__ __launch_bounds__(512) void probe(const f16x8* in, const float* fin, float* out, unsigned long long* ticks, int iters) {
    __shared__ __attribute__((aligned(16))) char lds[512 * 16];  // one 16-byte slot per thread: the ds_write_b128 filler's target
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    f16x8 a = in[lane], b = in[64 + lane];
    f32x4 c4[4];
    f32x16 c16[2];
    for (int t = 0; t < 4; ++t) for (int r = 0; r < 4; ++r) c4[t][r] = 0.f;
    for (int t = 0; t < 2; ++t) for (int r = 0; r < 16; ++r) c16[t][r] = 0.f;
    Regs R;
    for (int q = 0; q < 2; ++q) {  // random values in [0.5, 1.5); the multiplier is 1 so that they stay what they are
        const float* f = fin + (threadIdx.x * 2 + q) * 8;
        R.a[q] = f32x2{f[0], f[1]}; R.b[q] = f32x2{f[2], f[3]};
        R.s0[q] = f[0]; R.s1[q] = f[1]; R.t0[q] = f[2]; R.t1[q] = f[3];
        R.x0[q] = f[4]; R.x1[q] = -f[5]; R.m0[q] = f[6]; R.m1[q] = f[7]; R.r0[q] = 0.f; R.r1[q] = 0.f;
        R.h[q] = __builtin_bit_cast(unsigned, f[4]) >> 3; R.l[q] = 0;
        R.pa[q] = __builtin_bit_cast(unsigned, f[5]); R.pb[q] = __builtin_bit_cast(unsigned, f[6]);
    }
    R.k = 1.f;
    R.k2 = f32x2{1.f, 1.f};
    R.ld = u32x4{R.pa[0], R.pb[0], R.pa[1], R.pb[1]};
    R.laddr = threadIdx.x * 16;  // < sizeof(lds) for every thread of the 512 at most
    reinterpret_cast<u32x4*>(lds)[threadIdx.x] = R.ld;
    __syncthreads();
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    if constexpr (PLACE == P_SAME) {
        slots<SHAPE, FILL, NV, true, NV != 0>(R, c4, c16, a, b, iters);
    } else if (wave < 4) {
        if constexpr (PLACE == P_OTHER) slots<SHAPE, FILL, NV, true, false>(R, c4, c16, a, b, iters);
    } else {
        slots<SHAPE, FILL, NV, false, true>(R, c4, c16, a, b, iters);
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    float s = 0.f;
    for (int t = 0; t < 4; ++t) for (int r = 0; r < 4; ++r) s += c4[t][r];
    for (int t = 0; t < 2; ++t) for (int r = 0; r < 16; ++r) s += c16[t][r];
    for (int q = 0; q < 2; ++q)
        s += R.a[q][0] + R.b[q][1] + R.s0[q] + R.s1[q] + R.t0[q] + R.t1[q] + R.m0[q] + R.m1[q] + R.r0[q] + R.r1[q] + (float)(R.h[q] + R.l[q] + R.pa[q] + R.pb[q]);
    out[blockIdx.x * 512 + threadIdx.x] = s;
    if (blockIdx.x == 0 && lane == 0) ticks[wave] = c1 - c0;
}

#define CHECK(e)                                                                              \
    do {                                                                                      \
        const hipError_t err_ = (e);                                                          \
        if (err_ != hipSuccess) {                                                             \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_));      \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

struct Bufs {
    f16x8* in;
    float *fin, *out;
    unsigned long long* ticks;
    int blocks;
};

template <int SHAPE, int FILL, int NV, int PLACE>
static void run(const Bufs& B) {
    const int iters = 1600, threads = PLACE == P_SAME ? 256 : 512;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    float ms = 0;
    for (int rep = 0; rep < 2; ++rep) {  // (the first launch warms)
        CHECK(hipMemset(B.ticks, 0, 8 * sizeof(unsigned long long)));
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((probe<SHAPE, FILL, NV, PLACE>), dim3(B.blocks), dim3(threads), 0, 0, B.in, B.fin, B.out, B.ticks, iters);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipDeviceSynchronize());
        CHECK(hipEventElapsedTime(&ms, e0, e1));
    }
    unsigned long long t[8];
    CHECK(hipMemcpy(t, B.ticks, sizeof(t), hipMemcpyDeviceToHost));
    unsigned long long tm = 0, tv = 0;  // slowest wave of each role (s_memtime ticks)
    if (PLACE == P_SAME) {
        for (int w = 0; w < 4; ++w) tm = t[w] > tm ? t[w] : tm;
        tv = tm;
    } else {
        for (int w = 0; w < 4; ++w) tm = t[w] > tm ? t[w] : tm;
        for (int w = 4; w < 8; ++w) tv = t[w] > tv ? t[w] : tv;
        if (PLACE == P_ALONE) tm = 0;
    }
    const double slots = (double)iters * SLOTS, worst = (double)(tm > tv ? tm : tv);
    printf("{\"probe\": \"interleave_unpacked\", \"mfma\": \"%s\", \"filler\": \"%s\", \"n_per_mfma\": %d, \"placement\": \"%s\", \"blocks\": %d, "
           "\"clk_per_mfma_slot\": %.3f, \"clk_mfma_wave\": %.3f, \"clk_filler_wave\": %.3f, \"ns_kernel_per_slot\": %.3f}\n",
           SHAPE == 0 ? "16x16x32" : "32x32x16", NV == 0 ? "none" : FILL_NAME[FILL], NV, PLACE_NAME[PLACE], B.blocks, worst / slots,
           tm / slots, tv / slots, ms * 1e6 / slots);
    fflush(stdout);
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
}

template <int SHAPE, int FILL, int NV>
static void run_places(const Bufs& B) {
    run<SHAPE, FILL, NV, P_SAME>(B);
    run<SHAPE, FILL, NV, P_OTHER>(B);
    run<SHAPE, FILL, NV, P_ALONE>(B);
}
template <int SHAPE, int... FILL>
static void run_fills(const Bufs& B, std::integer_sequence<int, FILL...>) {
    run<SHAPE, F_MIX, 0, P_SAME>(B);  // the MFMA stream alone: M
    ((run_places<SHAPE, FILL, 2>(B), run_places<SHAPE, FILL, 4>(B), run_places<SHAPE, FILL, 6>(B)), ...);
}

int main() {
    Bufs B;
    CHECK(hipMalloc(&B.in, 128 * sizeof(f16x8)));
    CHECK(hipMalloc(&B.fin, 512 * 2 * 8 * sizeof(float)));
    CHECK(hipMalloc(&B.out, 256 * 512 * sizeof(float)));
    CHECK(hipMalloc(&B.ticks, 8 * sizeof(unsigned long long)));
    {
        srand(1);
        static _Float16 h[1024];
        for (int i = 0; i < 1024; ++i) h[i] = (_Float16)((rand() % 2001 - 1000) / 1000.f);
        CHECK(hipMemcpy(B.in, h, sizeof(h), hipMemcpyHostToDevice));
        static float f[512 * 2 * 8];
        for (int i = 0; i < 512 * 2 * 8; ++i) f[i] = 0.5f + (rand() % 100000) / 100000.f;
        CHECK(hipMemcpy(B.fin, f, sizeof(f), hipMemcpyHostToDevice));
        CHECK(hipMemset(B.out, 0, 256 * 512 * sizeof(float)));
    }
    for (int blocks : {1, 256}) {  // one CU (boost clock); every CU (power-limited clock)
        B.blocks = blocks;
        run_fills<1>(B, std::make_integer_sequence<int, F_COUNT>{});
        run_fills<0>(B, std::make_integer_sequence<int, F_COUNT>{});
    }
    return 0;
}
