// aligner.h -- the kernels of the forced aligner (reference utils/aligner/model.py:24-48, extract_durations.py:86-96,
// duration_extraction.py:52-85) that are not parrot_conv plans: the bidirectional LSTM recurrence, the masked softmax, the
// monotonic shortest-path dynamic programme, and the data movement around the conv plans (transpose, partial-sum / ReLU /
// BatchNorm-affine epilogue).  The five GEMMs -- three k = 5 convs, the LSTM input projection of both directions for all frames
// at once, the final Linear -- are parrot_conv plans owned by the parrot_aligner handle (host_aligner.hip).
// The launchers below are defined in tu_aligner.hip, which alone sees the kernel bodies (PARROT_ALIGNER_TU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace parrot {

constexpr int ALIGN_ST_NONFINITE = 5;  // a NaN / inf logit of a real frame (as the vocoder / TTE / mel handles use 5)
constexpr int ALIGN_ST_BAD_INPUT = 9;  // a token outside [0, V), or a mel_len / tokens_len outside [1, T] / [1, N]

constexpr int ALIGN_MAX_T = 32768;    // frames per utterance (back-pointer bytes: T x N per row of the batch)
constexpr int ALIGN_MAX_N = 2048;     // tokens per utterance: three fp64 anti-diagonals + the token ids in LDS (56 KiB)
constexpr int LSTM_MAX_DIM = 1024;    // lstm_dim: LSTM_BT rows of h in LDS (32 KiB)
constexpr int LSTM_UNITS = 4;         // hidden units per workgroup: 4 gates x 4 units = 16 weight rows, 16 k-lanes each
constexpr int LSTM_BT = 8;            // batch rows per pass over the workgroup's weight rows

struct LstmStepParams {
    const float* w_hh;    // [2][4H][H]: weight_hh_l0, weight_hh_l0_reverse (gate order i, f, g, o)
    const float* xproj;   // (B, T, 8H): W_ih x + b_ih + b_hh, forward gates then backward gates
    const float* h_prev;  // [2][B][H]
    float* h_next;        // [2][B][H]
    float* c;             // [2][B][H], updated in place
    float* out;           // (B, T, 2H): [forward, backward]
    int B, T, H, step;    // forward direction at t = step, backward at t = T - 1 - step
};

hipError_t launch_lstm_step(const LstmStepParams& p, hipStream_t s);
// steps 0 .. n_steps - 1 of the recurrence from (h0, c0) [2][B][H] (null: zeros) through hbuf [2][2][B][H] and q.c: the loop of
// parrot_aligner_forward (host_aligner.hip).  A PARROT_* code.
int lstm_run_steps(LstmStepParams q, float* hbuf, const float* h0, const float* c0, int n_steps, hipStream_t s);
// in (B, R, C) -> out (B, C, R)
hipError_t launch_align_transpose(const float* in, float* out, int B, int R, int C, hipStream_t s);
// out[b][c][t] = affine_c(relu?(sum_g in[b][g Mg + c][t])), in (B, G Mg, T), out (B, C, T) (may alias `in` when G == 1, Mg == C)
hipError_t launch_align_epilogue(const float* in, float* out, const float* scale, const float* shift, int B, int C, int T, int G, int Mg,
                                 int relu, hipStream_t s);
// logits (B, T, V) -> pred (B, T, V): softmax over V for t < mel_len[b] (clamped to [0, T]), zero beyond
hipError_t launch_align_softmax(const float* logits, const int32_t* mel_len, float* pred, int B, int T, int V, int* err, hipStream_t s);
hipError_t launch_align_dp(const float* pred, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, int B, int T, int V,
                           int N, uint8_t* bp, int32_t* dur, double* cost, int* status, hipStream_t s);

#ifdef PARROT_ALIGNER_TU

// ---------------------------------------------------------------------------------------------
// lstm_step_kernel: one launch advances both directions of the recurrence by one step (model.py:39 nn.LSTM, bidirectional,
// one layer).  grid (H / LSTM_UNITS, 2): workgroup (x, dir) owns hidden units [4x, 4x + 4) of direction dir and computes their
// four gates for every batch row.  Thread (r, q) = (tid / 16, tid % 16): weight row r = gate (r / 4) of unit 4x + r % 4, k-lane
// q: it adds w[k] h[k] over k = 4q .. 4q + 3, 4q + 64 .. in fp32 FMA, in that fixed order (16 accumulators of H / 16 products
// per dot product, then a fixed xor tree over the 16 lanes: no single chain over H), for LSTM_BT batch rows per pass with h in
// LDS.  Then one thread per (unit, row) adds the precomputed input projection, applies 1 / (1 + expf(-x)) and tanhf, updates c
// in place and writes h into the other half of the double buffer and into out[b][t].
// The only synchronisation between workgroups is stream order: step s + 1 is the next launch.  One code path for every H.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_step_kernel(const LstmStepParams p) {
    extern __shared__ float lstm_sm[];
    float* hs = lstm_sm;                      // [LSTM_BT][H]
    float* gates = lstm_sm + LSTM_BT * p.H;   // [16][LSTM_BT]
    const int H = p.H, B = p.B, T = p.T;
    const int dir = blockIdx.y, u0 = blockIdx.x * LSTM_UNITS, tid = threadIdx.x;
    const int t = dir ? T - 1 - p.step : p.step;
    const int r = tid >> 4, q = tid & 15;
    const float* __restrict__ wrow = p.w_hh + ((size_t)dir * 4 * H + (size_t)(r >> 2) * H + u0 + (r & 3)) * H;
    for (int b0 = 0; b0 < B; b0 += LSTM_BT) {
        const int nb = min(LSTM_BT, B - b0);
        for (int idx = tid; idx < LSTM_BT * H; idx += 256) {
            const int bb = idx / H;
            hs[idx] = bb < nb ? p.h_prev[((size_t)dir * B + b0 + bb) * H + (idx - bb * H)] : 0.f;
        }
        __syncthreads();
        float acc[LSTM_BT];
#pragma unroll
        for (int bb = 0; bb < LSTM_BT; ++bb) acc[bb] = 0.f;
        for (int k0 = 4 * q; k0 < H; k0 += 64) {  // (H % 16 == 0: k0 + 3 < H)
            const float4 w4 = *reinterpret_cast<const float4*>(wrow + k0);
#pragma unroll
            for (int bb = 0; bb < LSTM_BT; ++bb) {
                const float4 h4 = *reinterpret_cast<const float4*>(hs + bb * H + k0);
                acc[bb] = fmaf(w4.x, h4.x, acc[bb]);
                acc[bb] = fmaf(w4.y, h4.y, acc[bb]);
                acc[bb] = fmaf(w4.z, h4.z, acc[bb]);
                acc[bb] = fmaf(w4.w, h4.w, acc[bb]);
            }
        }
#pragma unroll
        for (int bb = 0; bb < LSTM_BT; ++bb) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc[bb] += __shfl_xor(acc[bb], o);  // (stays inside the row's 16 lanes)
            if (q == 0) gates[r * LSTM_BT + bb] = acc[bb];
        }
        __syncthreads();
        if (tid < LSTM_UNITS * LSTM_BT) {
            const int uu = tid & (LSTM_UNITS - 1), bb = tid / LSTM_UNITS;
            if (bb < nb) {
                const int b = b0 + bb, unit = u0 + uu;
                const float* __restrict__ xp = p.xproj + ((size_t)b * T + t) * 8 * H + (size_t)dir * 4 * H + unit;
                const float gi = xp[0] + gates[(0 * LSTM_UNITS + uu) * LSTM_BT + bb];
                const float gf = xp[H] + gates[(1 * LSTM_UNITS + uu) * LSTM_BT + bb];
                const float gg = xp[2 * H] + gates[(2 * LSTM_UNITS + uu) * LSTM_BT + bb];
                const float go = xp[3 * H] + gates[(3 * LSTM_UNITS + uu) * LSTM_BT + bb];
                const float i_ = 1.f / (1.f + expf(-gi)), f_ = 1.f / (1.f + expf(-gf)), g_ = tanhf(gg), o_ = 1.f / (1.f + expf(-go));
                const size_t ci = ((size_t)dir * B + b) * H + unit;
                // c = fma(f, c, fl32(i g)): two roundings, spelled out, here and in lstm_train_step_kernel alike.  (It used to read
                // __fadd_rn(__fmul_rn(f, c), __fmul_rn(i, g)); HIP's _rn intrinsics are a plain `*` and `+` under the default
                // -ffp-contract=fast, and the compiler fused one product into the add: f c here -- this very FMA -- but i g in the
                // training kernel, so the two kernels differed in the last bit of c.)
                const float cn = fmaf(f_, p.c[ci], i_ * g_);
                const float hn = o_ * tanhf(cn);
                p.c[ci] = cn;
                p.h_next[ci] = hn;
                p.out[((size_t)b * T + t) * 2 * H + (size_t)dir * H + unit] = hn;
            }
        }
        __syncthreads();  // (hs / gates are rewritten by the next pass)
    }
}

// ---------------------------------------------------------------------------------------------
// Batched transpose in (B, R, C) -> out (B, C, R) through a 32 x 32 LDS tile: reads contiguous in c, writes contiguous in r.
// grid (ceil(C / 32), ceil(R / 32), B).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void align_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int C) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const size_t base = (size_t)blockIdx.z * R * C;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < R && c0 + tx < C) tile[i][tx] = in[base + (size_t)(r0 + i) * C + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < C && r0 + tx < R) out[base + (size_t)(c0 + i) * R + r0 + tx] = tile[tx][i];
}

// ---------------------------------------------------------------------------------------------
// Conv epilogue: sum of the G channel-group partials of a grouped plan in group order (G = 1: the plain output), then ReLU,
// then the eval-mode BatchNorm as the per-channel affine v * scale[c] + shift[c] (model.py:16-19: conv -> relu -> bnorm), or a
// bias (scale == nullptr: v + shift[c]).  Elementwise: out may be `in` when G == 1.
// A non-finite sum becomes a NaN before the ReLU.  The conv plans store fmaxf(acc, -inf), which turns a NaN accumulator into
// -inf; a ReLU would make that 0 and the LSTM's gates would saturate on it, so a NaN mel value would end as finite logits.
// As a NaN it reaches every logit of its row through the recurrence and align_softmax_kernel raises ALIGN_ST_NONFINITE.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void align_epilogue_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, int C, int T, int G, int Mg, int relu, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T), c = (int)(i / T % C);
    const size_t b = i / ((size_t)T * C);
    float v = in[((b * G) * Mg + c) * T + t];
    for (int g = 1; g < G; ++g) v = __fadd_rn(v, in[((b * G + g) * Mg + c) * T + t]);
    if (!(fabsf(v) < INFINITY)) v = __int_as_float(0x7fc00000);  // (the plans' store hands a NaN accumulator on as -inf, see above)
    if (relu) v = v < 0.f ? 0.f : v;  // (a NaN stays a NaN, as torch's relu keeps it: fmaxf would drop it)
    if (scale) v = fmaf(v, scale[c], shift[c]);
    else if (shift) v = __fadd_rn(v, shift[c]);
    out[i] = v;
}

// ---------------------------------------------------------------------------------------------
// align_softmax_kernel: torch.softmax(logits[b, :mel_len[b]], -1) in fp32 (extract_durations.py:91-93): one wave per frame,
// max-shifted, expf, the sum over V by a fixed lane stride and a fixed xor tree.  Frames t >= mel_len[b] are written as zero and
// not examined; a non-finite logit of a real frame raises ALIGN_ST_NONFINITE.  A mel_len[b] outside [1, T] raises
// ALIGN_ST_BAD_INPUT (the larger status wins) and is clamped to [0, T], so nothing is read or written through it.  pred may be
// logits (in place).  grid ceil(B T / 4), 4 waves per workgroup.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void align_softmax_kernel(const float* logits, const int32_t* __restrict__ mel_len, float* pred, int B, int T, int V,
                                                            int* __restrict__ err) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)B * T) return;
    const int b = (int)(row / T), t = (int)(row % T);
    const int len = mel_len ? min(max(mel_len[b], 0), T) : T;
    if (mel_len && t == 0 && lane == 0 && (mel_len[b] < 1 || mel_len[b] > T)) atomicMax(err, ALIGN_ST_BAD_INPUT);
    const float* x = logits + row * V;  // (pred may be logits: a lane reads x[v] before it writes y[v], and no other lane's)
    float* y = pred + row * V;
    if (t >= len) {
        for (int v = lane; v < V; v += 64) y[v] = 0.f;
        return;
    }
    float m = -INFINITY;
    bool bad = false;
    for (int v = lane; v < V; v += 64) {
        const float a = x[v];
        bad |= !(fabsf(a) < INFINITY);
        m = fmaxf(m, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(x[v] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    for (int v = lane; v < V; v += 64) y[v] = expf(x[v] - m) / s;
    if (bad) atomicMax(err, ALIGN_ST_NONFINITE);
}

// ---------------------------------------------------------------------------------------------
// align_dp_kernel: extract_durations_with_dijkstra (duration_extraction.py:52-85) as the dynamic programme it is.  One workgroup
// per utterance b with its own T_b = mel_len[b], N_b = tokens_len[b]:
//   w[i][j]    = fl32(1 - pred[b][i][tokens[b][j]]), widened to fp64 (numpy subtracts in float32, scipy widens)
//   dist[0][0] = 0;  dist[i][j] = min(dist[i-1][j-1], dist[i-1][j], dist[i][j-1]) + w[i][j]   in fp64: the sum Dijkstra forms
// swept along the anti-diagonals i + j = d (independent cells), three of them in LDS indexed by j, one barrier per diagonal.
// Tie rule: on equal predecessor distances the diagonal wins, then the previous frame (i - 1, j), then the previous token
// (i, j - 1).  Back-pointers (one byte per cell: 0 diagonal, 1 previous frame, 2 previous token) go to bp (B, T, N); lane 0
// walks them back from (T_b - 1, N_b - 1): every frame counts for the LAST token visited in its row (duration_extraction.py:76-82),
// i.e. the cell through which the backward walk enters the row.  dur (B, N) int32 (zero beyond N_b), cost (B) = dist[T_b-1][N_b-1].
// The walk is confined to the grid whatever the distances are (NaN pred included): at j == 0 it goes up, at i == 0 left.
// A token outside [0, V) or a length outside [1, T] / [1, N] sets status ALIGN_ST_BAD_INPUT; that row's dur is zero and its cost
// NaN, and nothing is read through the bad value.  A NaN / inf probability among the gathered cells (all but (0, 0), whose weight
// no path pays) sets ALIGN_ST_NONFINITE; the larger status wins.  Dynamic LDS: 3 N doubles + N ints.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void align_dp_kernel(const float* __restrict__ pred, const int64_t* __restrict__ tokens, const int32_t* __restrict__ mel_len,
                                                       const int32_t* __restrict__ tokens_len, int T, int V, int N, uint8_t* __restrict__ bp,
                                                       int32_t* __restrict__ dur, double* __restrict__ cost, int* __restrict__ status) {
    extern __shared__ double dp_sm[];
    double* diag[3] = {dp_sm, dp_sm + N, dp_sm + 2 * N};
    int* tok = reinterpret_cast<int*>(dp_sm + 3 * N);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = mel_len[b], Nb = tokens_len[b];
    int bad = (Tb < 1 || Tb > T || Nb < 1 || Nb > N) ? 1 : 0;
    for (int j = tid; j < N; j += 256) {
        dur[(size_t)b * N + j] = 0;
        if (!bad && j < Nb) {
            const int64_t v = tokens[(size_t)b * N + j];
            if (v < 0 || v >= V) bad = 1;
            else tok[j] = (int)v;
        }
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            cost[b] = __longlong_as_double(0x7ff8000000000000LL);
            atomicMax(status, ALIGN_ST_BAD_INPUT);
        }
        return;
    }
    const float* __restrict__ pb = pred + (size_t)b * T * V;
    uint8_t* __restrict__ bpb = bp + (size_t)b * T * N;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    bool nonfinite = false;
    for (int d = 0; d <= Tb + Nb - 2; ++d) {
        double* cur = diag[d % 3];
        const double* p1 = diag[(d + 2) % 3];  // diagonal d - 1: (i - 1, j) at [j], (i, j - 1) at [j - 1]
        const double* p2 = diag[(d + 1) % 3];  // diagonal d - 2: (i - 1, j - 1) at [j - 1]
        const int jlo = max(0, d - (Tb - 1)), jhi = min(Nb - 1, d);
        for (int j = jlo + tid; j <= jhi; j += 256) {
            const int i = d - j;
            double dist = 0.0;
            int move = 0;
            if (d > 0) {
                const float pr = pb[(size_t)i * V + tok[j]];
                nonfinite |= !(fabsf(pr) < INFINITY);
                const double w = (double)__fsub_rn(1.0f, pr);
                const double dg = (i > 0 && j > 0) ? p2[j - 1] : inf;
                const double up = i > 0 ? p1[j] : inf;
                const double lf = j > 0 ? p1[j - 1] : inf;
                double best;
                if (j == 0) { best = up; move = 1; }
                else if (i == 0) { best = lf; move = 2; }
                else if (dg <= up && dg <= lf) { best = dg; move = 0; }
                else if (up <= lf) { best = up; move = 1; }
                else { best = lf; move = 2; }
                dist = best + w;
            }
            cur[j] = dist;
            bpb[(size_t)i * N + j] = (uint8_t)move;
        }
        __syncthreads();
    }
    if (nonfinite) atomicMax(status, ALIGN_ST_NONFINITE);
    if (tid == 0) {
        cost[b] = diag[(Tb + Nb - 2) % 3][Nb - 1];
        int i = Tb - 1, j = Nb - 1;
        int32_t* __restrict__ db = dur + (size_t)b * N;
        db[j] += 1;  // frame T_b - 1
        for (int n = 0; n < Tb + Nb && (i > 0 || j > 0); ++n) {
            int move = bpb[(size_t)i * N + j];
            if (j == 0) move = 1;
            else if (i == 0) move = 2;
            if (move == 2) --j;
            else {
                --i;
                if (move == 0) --j;
                db[j] += 1;  // the walk enters frame i at its last visited token
            }
        }
    }
}

#endif  // PARROT_ALIGNER_TU

}  // namespace parrot
