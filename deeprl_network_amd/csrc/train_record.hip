// Training record: one row per agent and update with what the reference writes to TensorBoard on every update (agents/policies.py:
// 40-48, 265-273: the three loss terms, their total, the learning rate, the gradient norm) plus critic diagnostics of the batch the
// update was computed from, appended to a device-resident ring behind the optimiser step.  Nothing is synchronised and nothing the
// update uses is written: the kernels only READ terms, grad_norm, lr_dev, R, Adv and the action bytes.
//
// SPECIFICATION (restated in float64 NumPy by tests/train_record_ref.py).  n = rows = T * E entries per agent; all sums
// are float64 over the agent's float32 entries, V = (double)R - (double)Adv is the value the return scan used (agents/utils.py
// _add_R_Adv); a row is rounded once to float32 when stored.  ring[slot = count % K][i][24]:
//    0 policy_loss   terms[i,0]                 1 value_loss  terms[i,1]              2 entropy_loss  terms[i,2]
//    3 total_loss    ((double)c0 + c1) + c2     4 lr          *lr_dev if given, else lr
//    5 gradnorm      grad_norm[min(i, G - 1)]   6 ret_mean    sum R / n               7 ret_std  sqrt(max(sum R^2 / n - ret_mean^2, 0))
//    8 value_mean    sum V / n                  9 explained_var  1 - (sum Adv^2 / n - (sum Adv / n)^2) / var_R, 0 where var_R <= 0
//   10 adv_mean      sum Adv / n               11 adv_std     sqrt(max(sum Adv^2 / n - adv_mean^2, 0))
//   12 entropy       -c2 / e_coef (mean policy entropy, nats; 0 if e_coef == 0)      13 rows  n        14, 15 reserved: 0
//   16 + a           share of the rows with action[r,i] == a for a < n_a[i] (n_a NULL: A), 0 for the other a
// then count += 1.  While *skip_if != 0 (the hand-off status word of a guarded model) neither launch writes anything: a batch whose
// in-launch hand-off timed out is refused and re-run by the host, so it leaves no row and does not advance the count.
//
// Mapping, two launches.  (1) partial: block c owns rows [c * rpc, min((c + 1) * rpc, rows)) of EVERY agent (rpc a multiple of 4,
// a function of rows alone).  R / Adv are agent-major: wave w of the block takes agents w, w + 8, ..., its 64 lanes stride over
// the chunk's rows of that agent -- coalesced 256-byte loads --, the five float64 partial sums are reduced by an xor butterfly in a
// fixed order and lane 0 stores them; nothing crosses a wave.  The action bytes are env-major: the chunk's rows are the contiguous
// bytes [c * rpc * N, ...), which the whole block reads as 4-byte words (coalesced; the agent of a byte is its offset mod N) and
// counts into one LDS histogram per wave with LDS integer atomics (order-independent), summed to the chunk's counts [N][8].
// (2) finish: ONE block of 1024 threads; the 13 N sums over the chunks (5 float64 sums and 8 action counts per agent) are tasks of 8
// adjacent lanes each: lane j adds the partials of the j-th eighth of the chunks in chunk order (its loads in flight together), an
// xor butterfly over the 8 lanes adds the eighths in a fixed order.  The block then forms the N x 24 row with contiguous stores,
// and thread 0 -- after a fence and a barrier -- stores count + 1: the increment is the last store of the call.  No floating-point atomics: a given (N, rows, A) gives the same bits on
// every run.  Algorithmic bytes: 9 N rows in (R, Adv, actions); 72 N chunks out and in again (workspace); 96 N out.
#include "common.h"

namespace {

constexpr int NMAX = 32;          // agents
constexpr int AMAX = 8;           // actions (the padded width of the heads, csrc/a2c.hip LOSS_MAXA)
constexpr int COLS = 24;          // floats of a row
constexpr int NSUM = 5;           // sum R, sum R^2, sum Adv, sum Adv^2, sum V
constexpr int WAVES = 8;          // waves per block of the partial kernel
constexpr int FIN_THREADS = 1024, FIN_LANES = 8;      // finish kernel: lanes per sum over the chunks
constexpr int MAX_CHUNKS = 256;
constexpr int MIN_CHUNK_ROWS = 256;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = NMARL_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, NMARL_WAVE);
    return v;
}

// common.h nmarl_ordered_sum for the float64 sums and the integer counts, over the chunks [c0, c1): p[c0 * stride] + ... in index
// order, the loads of U terms in flight together and only the adds serial.  Then the FIN_LANES adjacent lanes of a task add their
// pieces by an xor butterfly (fixed order; every lane of the task ends with the same bits).
template <typename T, int U = 16>
__device__ __forceinline__ T ordered_sum(const T* __restrict__ p, const int64_t stride, const int c0, const int c1) {
    T s = (T)0;
    for (int c = c0; c < c1; c += U) {
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = p[(int64_t)(c + u < c1 ? c + u : c1 - 1) * stride];
#pragma unroll
        for (int u = 0; u < U; ++u) if (c + u < c1) s += v[u];
    }
#pragma unroll
    for (int off = FIN_LANES / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, FIN_LANES);
    return s;
}

inline int64_t chunk_rows(int64_t rows) {
    int64_t rpc = (rows + MAX_CHUNKS - 1) / MAX_CHUNKS;
    rpc = rpc < MIN_CHUNK_ROWS ? MIN_CHUNK_ROWS : rpc;
    return (rpc + 3) / 4 * 4;
}

inline int chunks(int64_t rows) { return (int)((rows + chunk_rows(rows) - 1) / chunk_rows(rows)); }

__global__ __launch_bounds__(NMARL_WAVE * WAVES) void train_record_partial_kernel(
    const int N, const int64_t rows, const int64_t rpc, const float* __restrict__ R, const float* __restrict__ Adv,
    const uint8_t* __restrict__ action, const int32_t* __restrict__ skip_if, double* __restrict__ psum, uint32_t* __restrict__ phist) {
    if (skip_if != nullptr && *skip_if != 0) return;
    __shared__ uint32_t hist[WAVES][NMAX * AMAX];
    const int tid = threadIdx.x, lane = tid & (NMARL_WAVE - 1), wave = tid / NMARL_WAVE;
    for (int k = tid; k < WAVES * NMAX * AMAX; k += NMARL_WAVE * WAVES) (&hist[0][0])[k] = 0u;
    __syncthreads();
    const int64_t c = blockIdx.x, r0 = c * rpc, r1 = r0 + rpc < rows ? r0 + rpc : rows;

    for (int i = wave; i < N; i += WAVES) {
        const float* __restrict__ Ri = R + (int64_t)i * rows;
        const float* __restrict__ Ai = Adv + (int64_t)i * rows;
        double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
        for (int64_t r = r0 + lane; r < r1; r += NMARL_WAVE) {
            const double x = (double)Ri[r], a = (double)Ai[r];
            s[0] += x;
            s[1] += x * x;
            s[2] += a;
            s[3] += a * a;
            s[4] += x - a;
        }
#pragma unroll
        for (int k = 0; k < NSUM; ++k) s[k] = wave_sum(s[k]);
        if (lane == 0) {
            double* out = psum + (c * N + i) * NSUM;
#pragma unroll
            for (int k = 0; k < NSUM; ++k) out[k] = s[k];
        }
    }

    // the chunk's action bytes [r0 * N, r1 * N): r0 * N is a multiple of 4 (rpc is) and the base is 4-byte aligned (checked by the host)
    const int64_t b0 = r0 * N;
    const uint32_t nbytes = (uint32_t)((r1 - r0) * N), nwords = nbytes >> 2, first = (uint32_t)(b0 % N);
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(action + b0);
    uint32_t* h = hist[wave];
    for (uint32_t w = tid; w < nwords; w += NMARL_WAVE * WAVES) {
        const uint32_t v = words[w];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t a = (v >> (8 * j)) & 255u, agent = (first + 4 * w + j) % (uint32_t)N;
            if (a < AMAX) atomicAdd(&h[agent * AMAX + a], 1u);
        }
    }
    for (uint32_t b = (nwords << 2) + tid; b < nbytes; b += NMARL_WAVE * WAVES) {
        const uint32_t a = action[b0 + b], agent = (first + b) % (uint32_t)N;
        if (a < AMAX) atomicAdd(&h[agent * AMAX + a], 1u);
    }
    __syncthreads();
    for (int k = tid; k < N * AMAX; k += NMARL_WAVE * WAVES) {
        uint32_t t = 0u;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += hist[w][k];
        phist[c * N * AMAX + k] = t;
    }
}

struct RecordArgs {
    int64_t rows;
    int32_t N, A, G, K;
    float lr, e_coef;
    const int32_t* n_a;
    const float *terms, *grad_norm, *lr_dev;
    float* ring;
    int64_t* count;
    const int32_t* skip_if;
};

__global__ __launch_bounds__(FIN_THREADS) void train_record_finish_kernel(const RecordArgs a, const int C,
                                                                          const double* __restrict__ psum,
                                                                          const uint32_t* __restrict__ phist) {
    if (a.skip_if != nullptr && *a.skip_if != 0) return;
    __shared__ double s[NMAX][NSUM];
    __shared__ uint32_t h[NMAX][AMAX];
    const int tid = threadIdx.x, N = a.N;
    const int64_t cnt = *a.count;           // (read by every thread before the barriers; stored by thread 0 behind them)
    {
        // task t < N * NSUM: float64 sum t of psum [C][N * NSUM]; then count t - N * NSUM of phist [C][N * AMAX]
        const int j = tid % FIN_LANES, seg = (C + FIN_LANES - 1) / FIN_LANES;
        const int c0 = j * seg < C ? j * seg : C, c1 = c0 + seg < C ? c0 + seg : C;
        const int nd = N * NSUM, ntask = nd + N * AMAX;
        for (int t0 = 0; t0 < ntask; t0 += FIN_THREADS / FIN_LANES) {      // (trip count uniform over the block: the shuffles see whole tasks)
            const int t = t0 + tid / FIN_LANES;
            const bool live = t < ntask, dbl = t < nd;
            const double vd = ordered_sum(psum + (dbl ? t : 0), (int64_t)nd, live && dbl ? c0 : 0, live && dbl ? c1 : 0);
            const uint32_t vh = ordered_sum(phist + (live && !dbl ? t - nd : 0), (int64_t)N * AMAX, live && !dbl ? c0 : 0, live && !dbl ? c1 : 0);
            if (live && j == 0) {
                if (dbl) (&s[0][0])[t] = vd;
                else (&h[0][0])[t - nd] = vh;
            }
        }
    }
    __syncthreads();
    const int slot = (int)(cnt % a.K);
    float* __restrict__ out = a.ring + (int64_t)slot * N * COLS;
    const double n = (double)a.rows;
    for (int p = tid; p < N * COLS; p += FIN_THREADS) {
        const int i = p / COLS, col = p % COLS;
        const float c0 = a.terms[i * 3 + 0], c1 = a.terms[i * 3 + 1], c2 = a.terms[i * 3 + 2];
        const double ret_mean = s[i][0] / n, var_r = s[i][1] / n - ret_mean * ret_mean;
        const double adv_mean = s[i][2] / n, var_a = s[i][3] / n - adv_mean * adv_mean;
        float v = 0.0f;
        switch (col) {
            case 0: v = c0; break;
            case 1: v = c1; break;
            case 2: v = c2; break;
            case 3: v = (float)(((double)c0 + (double)c1) + (double)c2); break;
            case 4: v = a.lr_dev != nullptr ? *a.lr_dev : a.lr; break;
            case 5: v = a.grad_norm[i < a.G - 1 ? i : a.G - 1]; break;
            case 6: v = (float)ret_mean; break;
            case 7: v = (float)sqrt(var_r > 0.0 ? var_r : 0.0); break;
            case 8: v = (float)(s[i][4] / n); break;
            case 9: v = var_r > 0.0 ? (float)(1.0 - var_a / var_r) : 0.0f; break;
            case 10: v = (float)adv_mean; break;
            case 11: v = (float)sqrt(var_a > 0.0 ? var_a : 0.0); break;
            case 12: v = a.e_coef != 0.0f ? (float)(-(double)c2 / (double)a.e_coef) : 0.0f; break;
            case 13: v = (float)n; break;
            case 14:
            case 15: break;
            default: {
                const int act = col - 16, own = a.n_a != nullptr ? a.n_a[i] : a.A;
                v = act < own && act < a.A ? (float)((double)h[i][act] / n) : 0.0f;
            }
        }
        out[p] = v;
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) *a.count = cnt + 1;
}

inline bool sizes_ok(int32_t N, int64_t rows) { return N >= 1 && N <= NMAX && rows >= 1 && rows <= ((int64_t)1 << 31); }

}  // namespace

extern "C" int nmarl_train_record_ws_bytes(int32_t N, int64_t rows) {
    if (!sizes_ok(N, rows)) return NMARL_EINVAL;
    return chunks(rows) * N * (NSUM * (int)sizeof(double) + AMAX * (int)sizeof(uint32_t));
}

extern "C" int nmarl_train_record(const nmarl_train_record_t* p, void* stream) {
    if (!p || !sizes_ok(p->N, p->rows) || p->A < 1 || p->A > AMAX || p->G < 1 || p->G > p->N || p->K < 1) return NMARL_EINVAL;
    if (!p->terms || !p->grad_norm || !p->R || !p->Adv || !p->action || !p->ring || !p->count || !p->ws) return NMARL_EINVAL;
    if (((uintptr_t)p->action % 4) || ((uintptr_t)p->ws % 8) || ((uintptr_t)p->count % 8) || ((uintptr_t)p->skip_if % 4))
        return NMARL_EINVAL;
    const int C = chunks(p->rows);
    double* psum = static_cast<double*>(p->ws);
    uint32_t* phist = reinterpret_cast<uint32_t*>(psum + (int64_t)C * p->N * NSUM);
    RecordArgs a{};
    a.rows = p->rows; a.N = p->N; a.A = p->A; a.G = p->G; a.K = p->K; a.lr = p->lr; a.e_coef = p->e_coef;
    a.n_a = p->n_a; a.terms = p->terms; a.grad_norm = p->grad_norm; a.lr_dev = p->lr_dev;
    a.ring = p->ring; a.count = p->count; a.skip_if = p->skip_if;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(train_record_partial_kernel, dim3((unsigned)C), dim3(NMARL_WAVE * WAVES), 0, st, (int)p->N, p->rows,
                       chunk_rows(p->rows), p->R, p->Adv, p->action, p->skip_if, psum, phist);
    hipLaunchKernelGGL(train_record_finish_kernel, dim3(1), dim3(FIN_THREADS), 0, st, a, C, (const double*)psum, (const uint32_t*)phist);
    return nmarl_check_launch();
}
