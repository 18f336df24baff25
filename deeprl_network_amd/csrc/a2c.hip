// Pointwise / scan kernels of the A2C update path, agent-major [N, E, .] layout.
//
//   lstm_cell_{fwd,bwd}  gate maths of agents/utils.py:102-113 (lstm), 199-208
//                        (lstm_comm), 401-408 (lstm_ic3): done-masked state,
//                        gate order i,f,o,u, c' = f*c + i*u, h' = o*tanh(c').
//   sample_actions       utils.py:135-141 (np.random.choice == inverse CDF with one
//                        uniform; argmax in test mode), fused with the transposition
//                        to the env-major uint8 action array.
//   nstep_return         agents/utils.py:763-775 / 837-855 (global reward) and
//                        800-816 / 888-912 (spatially discounted), float64 scan.
//   rmsprop_tf_clip      policies.py:32-39, 257-264: tf.clip_by_global_norm +
//                        tf.train.RMSPropOptimizer (TF-1.12 ApplyRMSProp: ms0 = 1,
//                        epsilon inside the sqrt), over one flat parameter buffer.
// All HBM-bound elementwise/scan work: no MFMA.
#include "common.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// Every tensor is [N, E, W] with contiguous [E, W] panels and its own agent stride (floats), so that
// slot t of an [N, T, E, W] sequence buffer can be passed without a copy.
struct CellStrides { int64_t z, z2, bias, c_prev, gates, c_new, h_new, dh, dh2, dc, dz, dc_prev; };

// z: pre-activations WITHOUT bias; gates (out, optional): post-activation i,f,o,u;
// c_prev is masked by (1-done[e]) here.  4 hidden units per thread, 16-byte accesses.
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(
    const int64_t E, const int N, const int H, const CellStrides st, const float* __restrict__ z,
    const float* __restrict__ z2, const float* __restrict__ bias, const float* __restrict__ c_prev,
    const float* __restrict__ done, float* __restrict__ gates, float* __restrict__ c_new,
    float* __restrict__ h_new) {
    const int H4 = H >> 2;                                   // float4 groups per row
    const int64_t total = (int64_t)N * E * H4;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / H4;
        const int j = (int)(idx - row * H4) * 4;
        const int64_t n = row / E;
        const int64_t e = row - n * E;
        const float* zr = z + n * st.z + e * 4 * H;
        const float* b = bias + n * st.bias;
        float4 zi = *reinterpret_cast<const float4*>(zr + j), zf = *reinterpret_cast<const float4*>(zr + H + j);
        float4 zo = *reinterpret_cast<const float4*>(zr + 2 * H + j), zu = *reinterpret_cast<const float4*>(zr + 3 * H + j);
        if (z2 != nullptr) {      // x-side pre-activation kept separate: no copy+accumulate GEMM needed
            const float* yr = z2 + n * st.z2 + e * 4 * H;
            const float4 a = *reinterpret_cast<const float4*>(yr + j), b2 = *reinterpret_cast<const float4*>(yr + H + j);
            const float4 c2 = *reinterpret_cast<const float4*>(yr + 2 * H + j), d2 = *reinterpret_cast<const float4*>(yr + 3 * H + j);
            zi.x += a.x; zi.y += a.y; zi.z += a.z; zi.w += a.w;  zf.x += b2.x; zf.y += b2.y; zf.z += b2.z; zf.w += b2.w;
            zo.x += c2.x; zo.y += c2.y; zo.z += c2.z; zo.w += c2.w;  zu.x += d2.x; zu.y += d2.y; zu.z += d2.z; zu.w += d2.w;
        }
        const float4 bi = *reinterpret_cast<const float4*>(b + j), bf = *reinterpret_cast<const float4*>(b + H + j);
        const float4 bo = *reinterpret_cast<const float4*>(b + 2 * H + j), bu = *reinterpret_cast<const float4*>(b + 3 * H + j);
        const float4 cp = *reinterpret_cast<const float4*>(c_prev + n * st.c_prev + e * H + j);
        const float keep = 1.0f - done[e];
        float4 gi, gf, go, gu, c, h;
#define NMARL_CELL(k)                                              \
        gi.k = sigmoidf_(zi.k + bi.k); gf.k = sigmoidf_(zf.k + bf.k); \
        go.k = sigmoidf_(zo.k + bo.k); gu.k = tanhf(zu.k + bu.k);    \
        c.k = gf.k * (cp.k * keep) + gi.k * gu.k; h.k = go.k * tanhf(c.k);
        NMARL_CELL(x) NMARL_CELL(y) NMARL_CELL(z) NMARL_CELL(w)
#undef NMARL_CELL
        if (gates != nullptr) {
            float* gr = gates + n * st.gates + e * 4 * H;
            *reinterpret_cast<float4*>(gr + j) = gi; *reinterpret_cast<float4*>(gr + H + j) = gf;
            *reinterpret_cast<float4*>(gr + 2 * H + j) = go; *reinterpret_cast<float4*>(gr + 3 * H + j) = gu;
        }
        *reinterpret_cast<float4*>(c_new + n * st.c_new + e * H + j) = c;
        *reinterpret_cast<float4*>(h_new + n * st.h_new + e * H + j) = h;
    }
}

__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(
    const int64_t E, const int N, const int H, const CellStrides st, const float* __restrict__ gates,
    const float* __restrict__ c_prev, const float* __restrict__ c_new, const float* __restrict__ done,
    const float* __restrict__ dh, const float* __restrict__ dh2, const float* __restrict__ dc_in,
    float* __restrict__ dz, float* __restrict__ dc_prev) {
    const int H4 = H >> 2;
    const int64_t total = (int64_t)N * E * H4;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / H4;
        const int j = (int)(idx - row * H4) * 4;
        const int64_t n = row / E;
        const int64_t e = row - n * E;
        const float* gr = gates + n * st.gates + e * 4 * H;
        const float4 gi = *reinterpret_cast<const float4*>(gr + j), gf = *reinterpret_cast<const float4*>(gr + H + j);
        const float4 go = *reinterpret_cast<const float4*>(gr + 2 * H + j), gu = *reinterpret_cast<const float4*>(gr + 3 * H + j);
        const float4 cp = *reinterpret_cast<const float4*>(c_prev + n * st.c_prev + e * H + j);
        const float4 cn = *reinterpret_cast<const float4*>(c_new + n * st.c_new + e * H + j);
        const float4 zero = float4{0.f, 0.f, 0.f, 0.f};
        float4 gh = dh ? *reinterpret_cast<const float4*>(dh + n * st.dh + e * H + j) : zero;
        if (dh2 != nullptr) {     // recurrent part of dL/dh_t, kept apart from the head's part: no add pass
            const float4 g2 = *reinterpret_cast<const float4*>(dh2 + n * st.dh2 + e * H + j);
            gh.x += g2.x; gh.y += g2.y; gh.z += g2.z; gh.w += g2.w;
        }
        const float4 gcin = dc_in ? *reinterpret_cast<const float4*>(dc_in + n * st.dc + e * H + j) : zero;
        const float keep = 1.0f - done[e];
        float4 di, df, dO, du, dcp;
#define NMARL_CELLB(k)                                                          \
        { const float tc = tanhf(cn.k);                                          \
          const float g_c = gcin.k + gh.k * go.k * (1.0f - tc * tc);             \
          di.k = g_c * gu.k * gi.k * (1.0f - gi.k);                              \
          df.k = g_c * (cp.k * keep) * gf.k * (1.0f - gf.k);                     \
          dO.k = gh.k * tc * go.k * (1.0f - go.k);                               \
          du.k = g_c * gi.k * (1.0f - gu.k * gu.k);                              \
          dcp.k = g_c * gf.k * keep; }
        NMARL_CELLB(x) NMARL_CELLB(y) NMARL_CELLB(z) NMARL_CELLB(w)
#undef NMARL_CELLB
        float* dzr = dz + n * st.dz + e * 4 * H;
        *reinterpret_cast<float4*>(dzr + j) = di; *reinterpret_cast<float4*>(dzr + H + j) = df;
        *reinterpret_cast<float4*>(dzr + 2 * H + j) = dO; *reinterpret_cast<float4*>(dzr + 3 * H + j) = du;
        *reinterpret_cast<float4*>(dc_prev + n * st.dc_prev + e * H + j) = dcp;
    }
}

// x [N, rows, W] (agent stride x_sn) += bias [N, W] (stride bias_sn), then act: 0 none, 1 relu, 2 tanh.
// Replaces broadcast-copy + beta=1 GEMM + activation (3 passes) after a plain batched GEMM (fc of
// agents/utils.py:65-73 and the encoders of lstm_comm / lstm_ic3) in the no-grad rollout.
__global__ __launch_bounds__(256) void bias_act_kernel(const int64_t rows, const int N, const int W, const float* __restrict__ x,
                                                       const int64_t x_sn, const float* __restrict__ bias,
                                                       const int64_t bias_sn, const int act, float* __restrict__ y,
                                                       const int64_t y_sn, const int64_t y_row) {
    const int W4 = W >> 2;
    const int64_t total = (int64_t)N * rows * W4;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / W4;
        const int j = (int)(idx - row * W4) * 4;
        const int64_t n = row / rows;
        const int64_t r = row - n * rows;
        const float4 b = *reinterpret_cast<const float4*>(bias + n * bias_sn + j);
        float4 v = *reinterpret_cast<const float4*>(x + n * x_sn + r * W + j);
        v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
        if (act == 1) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        else if (act == 2) { v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w); }
        *reinterpret_cast<float4*>(y + n * y_sn + r * y_row + j) = v;
    }
}

// pi: [N, E, A] probabilities.  mode 0: inverse-CDF with uniforms u[E,N] (legacy host
// stream); mode 1: Philox(seed; env_id, agent>>2, step, ACTION); mode 2: argmax.  step = step_host + *step_dev.
__global__ __launch_bounds__(256) void sample_kernel(
    const int64_t E, const int N, const int A, const float* __restrict__ pi, const float* __restrict__ u,
    const int mode, const uint64_t seed, const int64_t env_id_base, const int64_t step_host,
    const int64_t* __restrict__ step_dev, uint8_t* __restrict__ action) {
    const int64_t total = E * N;
    const int64_t step = step_host + (step_dev ? *step_dev : 0);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = idx / N;
        const int n = (int)(idx - e * N);
        const float* p = pi + ((int64_t)n * E + e) * A;
        int a = 0;
        if (mode == 2) {
            float best = p[0];
            for (int k = 1; k < A; ++k) if (p[k] > best) { best = p[k]; a = k; }   // np.argmax: first max
        } else {
            float uu;
            if (mode == 0) {
                uu = u[idx];
            } else {
                const Philox4 r = philox4x32_10((uint32_t)(env_id_base + e), (uint32_t)(n >> 2), (uint32_t)step,
                                                NMARL_STREAM_ACTION, (uint32_t)seed, (uint32_t)(seed >> 32));
                const uint32_t w = (n & 3) == 0 ? r.x : (n & 3) == 1 ? r.y : (n & 3) == 2 ? r.z : r.w;
                uu = u01_from_bits(w);
            }
            // numpy: cdf = cumsum(double(p)); cdf /= cdf[-1]; searchsorted(cdf, u, side='right')
            double tot = 0.0;
            for (int k = 0; k < A; ++k) tot += (double)p[k];
            double cum = 0.0;
            for (int k = 0; k < A; ++k) {
                cum += (double)p[k];
                if (cum / tot <= (double)uu) a = k + 1;
            }
            if (a > A - 1) a = A - 1;
        }
        action[idx] = (uint8_t)a;
    }
}

// n-step return / advantage.  r: [T,E] (global) or [T,E,N] (per-agent, spatial);
// v: [T,N,E]; done_post: [T,E]; R_end: [N,E]; outputs R, Adv: [N,T,E].
// alpha < 0: R = r + gamma*R*(1-d).  alpha >= 0: R = gamma*R*(1-d) + sum_d alpha^d sum_{dist(i,j)=d} r_j.
__global__ __launch_bounds__(256) void nstep_kernel(
    const int64_t E, const int N, const int T, const float* __restrict__ r, const float* __restrict__ v,
    const uint8_t* __restrict__ done_post, const float* __restrict__ R_end, const double gamma,
    const double alpha, const int32_t* __restrict__ dist, float* __restrict__ R_out, float* __restrict__ adv_out) {
    __shared__ double s_w[64 * 64];  // alpha^dist(i,j), N <= 64
    const bool spatial = alpha >= 0.0;
    if (spatial) {
        // unreachable pairs (distance -1: directed Monaco graph, real_net_env.py:152-187) match no hop count -> weight 0
        for (int p = threadIdx.x; p < N * N; p += blockDim.x) s_w[p] = dist[p] < 0 ? 0.0 : pow(alpha, (double)dist[p]);
        __syncthreads();
    }
    const int64_t total = (int64_t)N * E;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(idx / E);
        const int64_t e = idx - (int64_t)n * E;
        double R = (double)R_end[idx];
        if (!spatial) {
            // the scan is one dependent multiply-add per step, its operands are not: ten steps' done / r / v are requested together
            // (one load latency per ten steps instead of per step: 60 -> 20 us at 8 x 4096 x 60, 97 -> 34 us at 25 x 1024 x 120); same arithmetic, same order
            constexpr int U = 10;
            for (int t0 = T - 1; t0 >= 0; t0 -= U) {
                float rr[U], vv[U];
                uint8_t dd[U];
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const int t = t0 - k >= 0 ? t0 - k : 0;                  // (clamped: unconditional loads)
                    dd[k] = done_post[(int64_t)t * E + e];
                    rr[k] = r[(int64_t)t * E + e];
                    vv[k] = v[((int64_t)t * N + n) * E + e];
                }
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const int t = t0 - k;
                    if (t < 0) break;
                    R = (double)rr[k] + gamma * R * (1.0 - (double)dd[k]);
                    const int64_t o = ((int64_t)n * T + t) * E + e;
                    R_out[o] = (float)R;
                    adv_out[o] = (float)(R - (double)vv[k]);
                }
            }
            continue;
        }
        for (int t = T - 1; t >= 0; --t) {
            const double keep = 1.0 - (double)done_post[(int64_t)t * E + e];
            R = gamma * R * keep;
            const float* rt = r + ((int64_t)t * E + e) * N;
            double add = 0.0;
            for (int j = 0; j < N; ++j) add += s_w[n * N + j] * (double)rt[j];
            R += add;
            const int64_t o = ((int64_t)n * T + t) * E + e;
            R_out[o] = (float)R;
            adv_out[o] = (float)(R - (double)v[((int64_t)t * N + n) * E + e]);
        }
    }
}

// GAE(lambda) advantage and lambda-return (opt-in, MODEL_CONFIG gae_lambda; the reference has no lambda).  Layouts of nstep_kernel.
//   rho[t] = r[t,e] (alpha < 0)  |  sum_j alpha^dist(n,j) r[t,e,j] (alpha >= 0, j ascending);  next = R_end, A = 0;  t = T-1 .. 0:
//   delta = rho[t] + (gamma next) keep - v[t];  A = delta + ((gamma lambda) A) keep;  Adv = A;  R = A + v[t];  next = v[t]
// Only A is a dependent chain: ten steps' done / r / v are requested together as in nstep_kernel, v[t] is loaded once and serves as
// the subtrahend at t and, from its register, as `next` at t - 1 (the bytes nstep_kernel moves).  Spatial path: the ten steps'
// weighted sums run side by side (ten independent loads and accumulators per j, each sum over j ascending).  One instantiation
// per path: a run-time `spatial` inside the unrolled loads made the compiler wait for each of them on its own.
template <bool SPATIAL>
__global__ __launch_bounds__(256) void gae_kernel(
    const int64_t E, const int N, const int T, const float* __restrict__ r, const float* __restrict__ v,
    const uint8_t* __restrict__ done_post, const float* __restrict__ R_end, const double gamma, const double lambda,
    const double alpha, const int32_t* __restrict__ dist, float* __restrict__ R_out, float* __restrict__ adv_out) {
    __shared__ double s_w[SPATIAL ? 64 * 64 : 1];  // alpha^dist(i,j), N <= 64
    if (SPATIAL) {
        for (int p = threadIdx.x; p < N * N; p += blockDim.x) s_w[p] = dist[p] < 0 ? 0.0 : pow(alpha, (double)dist[p]);
        __syncthreads();
    }
    const double gl = gamma * lambda;
    const int64_t total = (int64_t)N * E;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(idx / E);
        const int64_t e = idx - (int64_t)n * E;
        double next = (double)R_end[idx], A = 0.0;
        constexpr int U = 10;
        for (int t0 = T - 1; t0 >= 0; t0 -= U) {
            float vv[U], rr[U];
            uint8_t dd[U];
            double rho[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int t = t0 - k >= 0 ? t0 - k : 0;                  // (clamped: unconditional loads)
                dd[k] = done_post[(int64_t)t * E + e];
                vv[k] = v[((int64_t)t * N + n) * E + e];
                if (!SPATIAL) rr[k] = r[(int64_t)t * E + e];
            }
            if (SPATIAL) {
                const float* rk[U];
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    rk[k] = r + ((int64_t)(t0 - k >= 0 ? t0 - k : 0) * E + e) * N;
                    rho[k] = 0.0;
                }
                const double* w = s_w + n * N;
                // four neighbouring j per step at a time: a replica's row of N rewards is contiguous, so the four loads share a cache
                // line, where ten steps' single loads per j brought ten lines per thread back for every j (more than the L1 holds).
                // Each step's sum still runs over j ascending
                constexpr int JB = 4;
                int j = 0;
                for (; j + JB <= N; j += JB) {
                    float x[U][JB];
#pragma unroll
                    for (int k = 0; k < U; ++k)
#pragma unroll
                        for (int b = 0; b < JB; ++b) x[k][b] = rk[k][j + b];
#pragma unroll
                    for (int b = 0; b < JB; ++b) {
                        const double wj = w[j + b];
#pragma unroll
                        for (int k = 0; k < U; ++k) rho[k] += wj * (double)x[k][b];
                    }
                }
                for (; j < N; ++j) {                                     // the last N % 4: ten loads in flight per j
                    const double wj = w[j];
#pragma unroll
                    for (int k = 0; k < U; ++k) rr[k] = rk[k][j];
#pragma unroll
                    for (int k = 0; k < U; ++k) rho[k] += wj * (double)rr[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < U; ++k) rho[k] = (double)rr[k];
            }
            // straight-line over the ten steps; behind t = 0 (last chunk only) the clamped operands are scanned and not stored
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int t = t0 - k;
                const double keep = 1.0 - (double)dd[k], vt = (double)vv[k];
                const double delta = rho[k] + (gamma * next) * keep - vt;
                A = delta + (gl * A) * keep;
                if (t >= 0) {
                    const int64_t o = ((int64_t)n * T + t) * E + e;
                    adv_out[o] = (float)A;
                    R_out[o] = (float)(A + vt);
                }
                next = vt;
            }
        }
    }
}

// ---- clip_by_global_norm + RMSProp over flat [G, P] (G groups = optimisers) ----
// ---------------------------------------------------------------------------------------------------------------------
// What the batched loop does between two n_step batches, in two launches instead of ~45 elementwise ones:
//   (1) episode statistics of the reference's Trainer.run (utils.py:228-229, 253: mean / std of an episode's global
//       rewards), kept per replica across batches and closed where done is set; an episode shorter than T_env ended in
//       a collision (cacc_env.py:231-233);
//   (2) the state hand-over of the next `env.reset(); model.reset()` (utils.py:215-217; policies.py:151-154; cacc_env.py:184)
//       for the replicas that finished, and of `states_bw <- states_fw` (policies.py:115) / "slot T of the rollout buffers
//       is slot 0 of the next batch" for all.
struct EpilogueArgs {
    int64_t E;
    int32_t N, H, A, F, T, T_env;
    const float* g;
    const uint8_t* done;
    double *ep_sum, *ep_sq, *ep_len, *fin;
    float *h_fw, *c_fw, *h_bw, *c_bw;
    const float *fp_T, *fp_uniform, *x_T;
    float *fp_0, *x_0, *done_pre;
    const int32_t* skip_if;      // != NULL and *skip_if != 0: both kernels return without touching anything
};

constexpr int EPI_BLOCK = 256;
constexpr int EPI_MAX_BLOCKS = 1024;

// per-replica float64 sums in the order t = 0 .. T-1 (one thread per replica), a fixed-order tree over the block's
// replicas; the per-block partials are added in block order by the state kernel that follows (deterministic)
__global__ __launch_bounds__(EPI_BLOCK) void epilogue_stats_kernel(const EpilogueArgs a, double* __restrict__ partial) {
    if (a.skip_if && *a.skip_if != 0) return;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0, f3 = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * EPI_BLOCK + threadIdx.x; e < a.E; e += (int64_t)gridDim.x * EPI_BLOCK) {
        double s = 0.0, q = 0.0;
        constexpr int U = 12;                          // twelve steps' rewards requested together (one load latency per twelve steps); sums in
        for (int t0 = 0; t0 < a.T; t0 += U) {          // the same order t = 0 .. T-1
            float gv[U];
#pragma unroll
            for (int k = 0; k < U; ++k) gv[k] = a.g[(int64_t)(t0 + k < a.T ? t0 + k : a.T - 1) * a.E + e];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                if (t0 + k >= a.T) break;
                const double v = (double)gv[k];
                s += v;
                q += v * v;
            }
        }
        const double sum = a.ep_sum[e] + s, sq = a.ep_sq[e] + q, len = a.ep_len[e] + (double)a.T;
        const bool d = a.done[e] != 0;
        if (d) {
            const double mean = sum / len;
            double var = sq / len - mean * mean;
            var = var < 0.0 ? 0.0 : var;
            f0 += 1.0;
            f1 += mean;
            f2 += sqrt(var);
            f3 += len < (double)a.T_env ? 1.0 : 0.0;
        }
        a.ep_sum[e] = d ? 0.0 : sum;
        a.ep_sq[e] = d ? 0.0 : sq;
        a.ep_len[e] = d ? 0.0 : len;
    }
    __shared__ double red[4][EPI_BLOCK];
    red[0][threadIdx.x] = f0; red[1][threadIdx.x] = f1; red[2][threadIdx.x] = f2; red[3][threadIdx.x] = f3;
    __syncthreads();
    for (int off = EPI_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) partial[blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void epilogue_state_kernel(const EpilogueArgs a, const double* __restrict__ partial, const int n_partial) {
    if (a.skip_if && *a.skip_if != 0) return;
    if (blockIdx.x == 0 && threadIdx.x < 4) {          // episode statistics: the stats kernel's per-block partials, in block order
        double v = 0.0;
        for (int b = 0; b < n_partial; ++b) v += partial[b * 4 + threadIdx.x];
        a.fin[threadIdx.x] += v;
    }
    const int64_t nh = (int64_t)a.N * a.E * a.H, na = (int64_t)a.N * a.E * a.A, nx = a.E * (int64_t)a.N * a.F;
    const int64_t total = nh > na ? (nh > nx ? nh : nx) : (na > nx ? na : nx);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < nh) {                                  // [N][E][H]: recurrent state, zero where an episode ended
            const int64_t e = (i / a.H) % a.E;
            const float keep = a.done[e] ? 0.0f : 1.0f;
            const float h = a.h_fw[i] * keep, c = a.c_fw[i] * keep;
            a.h_fw[i] = h; a.h_bw[i] = h;
            a.c_fw[i] = c; a.c_bw[i] = c;
        }
        if (i < na) {                                  // [N][E][A]: fingerprints, uniform where an episode ended
            const int64_t e = (i / a.A) % a.E, n = i / (a.A * a.E);
            a.fp_0[i] = a.done[e] ? a.fp_uniform[n * a.A + (i % a.A)] : a.fp_T[i];
        }
        if (i < nx) a.x_0[i] = a.x_T[i];               // the env wrote the next observation (after its auto-reset)
        if (i < a.E) a.done_pre[i] = a.done[i] ? 1.0f : 0.0f;
    }
}

constexpr int SUMSQ_BLOCKS = 64;   // partial sums per group

// One block's partial sum of squares of its group's gradient (block x of SUMSQ_BLOCKS, group y): shared by both optimiser entries,
// so that the norm they report for the same g has the same bits.  block_dim / grid_dim: the kernel's blockDim.x / gridDim.x, read in
// the kernel (where the compiler knows the blocks to be uniform: sumsq_kernel keeps the instructions it had with the body in place).
__device__ __forceinline__ void sumsq_block(const int64_t P, const float* __restrict__ g, float* __restrict__ partial,
                                            const unsigned block_dim, const unsigned grid_dim) {
    const int grp = blockIdx.y;
    const float* gp = g + (int64_t)grp * P;
    float s = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * block_dim + threadIdx.x; i < P; i += (int64_t)grid_dim * block_dim) {
        const float x = gp[i];
        s += x * x;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ float sw[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sw[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[grp * SUMSQ_BLOCKS + blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

// Fail closed: a hand-off kernel of this batch reported a wave that gave up waiting (status[0] != 0, see nmarl_handoff_status in
// nmarl.h) -- its gradients are invalid, so an optimiser step applies NOTHING: weights and slots keep their values, the skipped
// update is counted (status[1], from one thread of the launch) and the host re-runs the batch on the launch-per-step path.
__device__ __forceinline__ bool status_raised(const int32_t* status) {
    return status && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

__device__ __forceinline__ bool step_refused(int32_t* status) {
    if (!status_raised(status)) return false;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(status + 1, 1);
    return true;
}

__global__ __launch_bounds__(256) void sumsq_kernel(const int64_t P, const float* __restrict__ g,
                                                    float* __restrict__ partial /*[G, SUMSQ_BLOCKS]*/) {
    sumsq_block(P, g, partial, blockDim.x, gridDim.x);
}

__global__ __launch_bounds__(256) void rmsprop_kernel(
    const int64_t P, float* __restrict__ w, const float* __restrict__ g, float* __restrict__ ms,
    const float* __restrict__ partial, const float* __restrict__ lr_ptr, const float lr_host, const float rho,
    const float eps, const float max_norm, const float grad_scale, float* __restrict__ norm_out, int32_t* status) {
    const int grp = blockIdx.y;
    if (step_refused(status)) return;
    // every block re-reduces its group's 64 partials in the same fixed order
    const float tot = nmarl_ordered_sum(partial + grp * SUMSQ_BLOCKS, 1, SUMSQ_BLOCKS);
    const float norm = sqrtf(tot) * fabsf(grad_scale);
    float scale = grad_scale;
    if (max_norm > 0.0f) scale = grad_scale * (max_norm * fminf(1.0f / norm, 1.0f / max_norm));
    const float lr = lr_ptr ? *lr_ptr : lr_host;
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[grp] = norm;
    const int64_t base = (int64_t)grp * P;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
        const float gc = g[base + i] * scale;
        float m = ms[base + i];
        m = m + (gc * gc - m) * (1.0f - rho);                 // ApplyRMSProp
        ms[base + i] = m;
        w[base + i] = w[base + i] - lr * gc / sqrtf(m + eps);
    }
}

// Opt-in Adam (Kingma & Ba) behind the same clip, nmarl_adam_clip[_guarded].  Two launches like RMSProp.  The step counter lives on
// the device (a replayed graph re-sends the host's arguments): the FIRST launch advances it, from one thread and only when the guard
// lets the step through; the SECOND only reads it -- no launch reads it for the bias correction and writes it.
__global__ __launch_bounds__(256) void adam_sumsq_kernel(const int64_t P, const float* __restrict__ g, float* __restrict__ partial,
                                                         int32_t* __restrict__ step, const int32_t* status) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && !status_raised(status))
        step[0] = step[0] + 1;                         // a refused batch keeps t (the host re-runs it)
    sumsq_block(P, g, partial, blockDim.x, gridDim.x);
}

__global__ __launch_bounds__(256) void adam_kernel(
    const int64_t P, float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m1, float* __restrict__ m2,
    const float* __restrict__ partial, const int32_t* __restrict__ step, const float* __restrict__ lr_ptr, const float lr_host,
    const float beta1, const float beta2, const float eps, const float max_norm, const float grad_scale,
    float* __restrict__ norm_out, int32_t* status) {
    const int grp = blockIdx.y;
    if (step_refused(status)) return;                  // w, m, v keep their bits (and adam_sumsq_kernel left the counter alone)
    // bias corrections 1 - beta^t, once per block in float64 (t = the counter the first launch advanced), then broadcast
    __shared__ float bc[2];
    if (threadIdx.x == 0) {
        const double t = (double)step[0];
        const double lr = (double)(lr_ptr ? *lr_ptr : lr_host);
        bc[0] = (float)(lr / (1.0 - pow((double)beta1, t)));                 // lr / (1 - beta1^t)
        bc[1] = (float)(1.0 / sqrt(1.0 - pow((double)beta2, t)));            // 1 / sqrt(1 - beta2^t)
    }
    __syncthreads();
    const float step_size = bc[0], rs_bc2 = bc[1];
    const float tot = nmarl_ordered_sum(partial + grp * SUMSQ_BLOCKS, 1, SUMSQ_BLOCKS);
    const float norm = sqrtf(tot) * fabsf(grad_scale);
    float scale = grad_scale;
    if (max_norm > 0.0f) scale = grad_scale * (max_norm * fminf(1.0f / norm, 1.0f / max_norm));
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[grp] = norm;
    const float c1 = 1.0f - beta1, c2 = 1.0f - beta2;
    const int64_t base = (int64_t)grp * P;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
        const float gc = g[base + i] * scale;
        const float m = beta1 * m1[base + i] + c1 * gc;
        const float v = beta2 * m2[base + i] + c2 * (gc * gc);
        m1[base + i] = m;
        m2[base + i] = v;
        w[base + i] = w[base + i] - step_size * m / (sqrtf(v) * rs_bc2 + eps);   // eps OUTSIDE the root
    }
}

// ---- per-batch advantage standardisation over [G, rows] (opt-in, MODEL_CONFIG adv_norm; the reference has none) ----
//   mu = mean x;  sigma = sqrt(mean (x - mu)^2) (population);  y = (x - mu) / (sigma + eps), eps OUTSIDE the root
// in float64 on the fp32 inputs, one rounding to fp32 on the store.  Two launches like sumsq_kernel / rmsprop_kernel, the caller's
// `partial` [G, chunks, 3] between them; a group's rows are cut into `chunks` contiguous pieces of `per` = ceil(rows / chunks).
//   (1) standardize_moments_kernel: block (chunk, group) -> the sum, the mean and M2 of its piece, two passes over the piece (the
//       sums, then the squares of the centred values: never E[x^2] - mu^2); the second pass re-reads what the first just brought
//       into the cache;
//   (2) standardize_apply_kernel: every block adds its group's sums and merges its (count, mean, M2) by Chan's formula in one fixed
//       tree, block 0 of a group writes (mu, sigma), each block writes y for its piece.
// The means Chan's formula works on are kept RELATIVE TO THE GROUP'S FIRST ELEMENT K = x[g, 0]: x - K is exact in float64 for fp32
// values of like magnitude, and the difference of two chunk means -- the term the formula squares -- then carries the rounding of
// numbers of the size of the spread, not of the size of the offset (advantages at 3e4 +- 1e-2: with plain means the rounding of
// each mean, 4e-12, against differences of ~1e-3 leaves sigma good to ~1e-11 at any chunking; relative to K it is good to ~1e-15).
// The variance does not see the shift.  mu does not go through K (K + a mean relative to K cancels where the data are centred and
// K is an outlying value): it is the plain sum over rows, the chunks' plain sums added in the same tree.  A triple in `partial` is
// (sum, mean - K, M2): the count of a chunk follows from (rows, per, chunk), and only the first launch, which writes nothing to y,
// reads K -- in place, x[g, 0] is overwritten by the second.
// 4-byte accesses in (1): the order of every sum is a function of (rows, chunks) alone, not of where a group starts (a dense pitch
// with odd rows puts group bases off 16 bytes); (2) has no order to keep and moves 16 bytes per lane between the peeled ends.
constexpr int STD_MAX_CHUNKS = 512;                 // slots of the merge tree: 2 per thread of a 256-thread block

// Sum over the block in a fixed order (lanes by shuffle, then the four waves), returned to every thread.  `sw`: 4 doubles of LDS
// per call site (no barrier between two uses of the same words).
__device__ __forceinline__ double std_block_sum(double s, double* sw) {
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

// rows of chunk c: per, fewer in the last chunk that has any, 0 behind it (rows < chunks happens)
__device__ __forceinline__ int64_t std_chunk_rows(const int64_t rows, const int64_t per, const int64_t c) {
    const int64_t left = rows - c * per;
    return left < per ? (left > 0 ? left : 0) : per;
}

__global__ __launch_bounds__(256) void standardize_moments_kernel(const int64_t rows, const int64_t per, const float* __restrict__ x,
                                                                  const int64_t x_sg, double* __restrict__ partial) {
    const int64_t n = std_chunk_rows(rows, per, blockIdx.x);
    const float* xg = x + (int64_t)blockIdx.y * x_sg;
    const float* xp = xg + (int64_t)blockIdx.x * per;
    const double K = (double)xg[0];
    __shared__ double sw[3][4];
    double s = 0.0, ps = 0.0;
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double v = (double)xp[i];
        ps += v;
        s += v - K;
    }
    const double sum = std_block_sum(ps, sw[2]);
    const double tot = std_block_sum(s, sw[0]);
    const double mean = n > 0 ? tot / (double)n : 0.0;                  // (of x - K)
    double q = 0.0;
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double d = ((double)xp[i] - K) - mean;
        q += d * d;
    }
    const double m2 = std_block_sum(q, sw[1]);
    if (threadIdx.x == 0) {
        double* p = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        p[0] = sum; p[1] = mean; p[2] = m2;
    }
}

struct StdMoments { double n, sum, mean, m2; };    // sum: of x;  mean: of x - K

// Chan, Golub & LeVeque: the moments of A followed by B (and the plain sums added).  An empty side is a no-op (no 0 / 0).
__device__ __forceinline__ StdMoments std_merge(const StdMoments a, const StdMoments b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, delta = b.mean - a.mean;
    return StdMoments{n, a.sum + b.sum, a.mean + delta * (b.n / n), (a.m2 + b.m2) + (delta * delta) * (a.n * (b.n / n))};
}

__global__ __launch_bounds__(256) void standardize_apply_kernel(const int64_t rows, const int64_t per, const float* x, const int64_t x_sg,
                                                                float* y, const int64_t y_sg, const double eps,
                                                                const double* __restrict__ partial, double* __restrict__ moments) {
    const int grp = blockIdx.y, C = gridDim.x, tid = threadIdx.x;
    const double* p = partial + (int64_t)grp * C * 3;
    // the group's C triples in one fixed tree over STD_MAX_CHUNKS slots (slot c = chunk c, empty behind C): slot t with t + 256, then
    // halving strides in LDS -- the same in every block of the group.  Every block of a group repeats the merge (up to 12 KB of
    // triples read from the cache and nine merge levels per block, ~6 MB of cache reads per call at 512 blocks): block 0 alone
    // could hand the result to the others only through a third launch, which costs more than the repeats
    __shared__ StdMoments sm[256];
    {
        StdMoments a{0.0, 0.0, 0.0, 0.0}, b{0.0, 0.0, 0.0, 0.0};
        if (tid < C) a = StdMoments{(double)std_chunk_rows(rows, per, tid), p[tid * 3], p[tid * 3 + 1], p[tid * 3 + 2]};
        if (tid + 256 < C)
            b = StdMoments{(double)std_chunk_rows(rows, per, tid + 256), p[(tid + 256) * 3], p[(tid + 256) * 3 + 1], p[(tid + 256) * 3 + 2]};
        sm[tid] = std_merge(a, b);
    }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sm[tid] = std_merge(sm[tid], sm[tid + off]);
        __syncthreads();
    }
    const double mu = sm[0].sum / (double)rows, sigma = sqrt(sm[0].m2 / (double)rows);
    if (blockIdx.x == 0 && tid == 0 && moments) {
        moments[grp * 2] = mu;
        moments[grp * 2 + 1] = sigma;
    }
    // y = (x - mu) * (1 / (sigma + eps)) in float64: the quotient of the definition to one more float64 rounding, far inside
    // the one fp32 rounding of the store; sigma = 0 with eps > 0 gives exact zeros, 0 * inf = NaN where the definition has 0 / 0
    const double inv = 1.0 / (sigma + eps);
#define NMARL_STD(v) (float)(((double)(v) - mu) * inv)
    const int64_t n = std_chunk_rows(rows, per, blockIdx.x);
    const float* xp = x + (int64_t)grp * x_sg + (int64_t)blockIdx.x * per;     // (no __restrict__: y == x is allowed; every element is
    float* yp = y + (int64_t)grp * y_sg + (int64_t)blockIdx.x * per;           //  read, then written, by one thread)
    const uintptr_t xa = reinterpret_cast<uintptr_t>(xp), ya = reinterpret_cast<uintptr_t>(yp);
    if (((xa ^ ya) & 15u) == 0) {
        // the same peel aligns both: up to 3 floats in front, float4 in the middle, up to 3 behind
        int64_t head = (int64_t)(((16u - (unsigned)(xa & 15u)) & 15u) >> 2);
        head = head < n ? head : n;
        const int64_t n4 = (n - head) >> 2;
        if (tid < head) yp[tid] = NMARL_STD(xp[tid]);
        const float4* x4 = reinterpret_cast<const float4*>(xp + head);
        float4* y4 = reinterpret_cast<float4*>(yp + head);
        for (int64_t i = tid; i < n4; i += 256) {
            const float4 v = x4[i];
            float4 o;
            o.x = NMARL_STD(v.x); o.y = NMARL_STD(v.y); o.z = NMARL_STD(v.z); o.w = NMARL_STD(v.w);
            y4[i] = o;
        }
        const int64_t done = head + (n4 << 2);
        if (done + tid < n) yp[done + tid] = NMARL_STD(xp[done + tid]);
    } else {
        for (int64_t i = tid; i < n; i += 256) yp[i] = NMARL_STD(xp[i]);
    }
#undef NMARL_STD
}

// ---- running return-based reward scaling (opt-in, MODEL_CONFIG reward_scale = return; the reference has none) ----
// S = E (global reward [T,E]) or E * N (per-agent reward [T,E,N]) reward streams, stream s of replica e = s (/ N).  Per call:
//   for t = 0..T-1: carry[s] = gamma carry[s] + r[t,s];  sample x = carry[s];  if done_post[t,e]: carry[s] = 0 (after the sample)
//   (n, mean, M2) <- the running population moments merged with the call's T S samples;  sigma = sqrt(M2 / n)
//   scale = sigma > 0 ? 1 / (sigma + eps) : 1;  r_out = fp32(double(r) scale), then clamped to +-clip if clip > 0
// all in float64.  THREE launches, the caller's `partial` [chunks, 4] and `state` [NMARL_REWARD_SCALE_STATE] between them:
//   (1) reward_scale_scan_kernel: one lane per stream (stream fastest in r: every load of r[t, .] coalesced), block b takes streams
//       b 256 + lane and then, past chunks x 256 streams, every (chunks 256)-th one behind it in ascending order; each lane runs
//       Welford over its own samples; lanes -> waves -> block by Chan's formula in one fixed order (shuffles, then the four waves);
//       one (n, sum, mean - K, M2) per block to `partial`; carry[s] is read and written by the one lane that owns s;
//   (2) reward_scale_merge_kernel, ONE block: the partials in one fixed tree (std_merge), then prior state + batch, the new state;
//   (3) reward_scale_apply_kernel: r_out from `scale` in the state.
// The running state is read and written by the same call.  Chosen: the one-block merge launch between scan and apply is the ONLY
// writer of `state`; (1) reads the state of before the call (n and K), (3) the state of after it, and launches on a stream run in
// order -- so no block can read a word another block of the same launch writes.  (Separate in / out words with a commit point would
// save a launch of ~2 us and need a second buffer whose roles swap per call: a replayed graph holds fixed addresses, so the swap
// would have to be a device-side index, one more word to get wrong.)
// Chan's means are kept relative to K, fixed for the life of the state: the first raw reward r[0, 0] of the first call on an empty
// state (n = 0) -- the first sample ever where the carry starts at 0 --, kept in the state; x - K carries the rounding of the spread,
// not of the offset (standardize_moments_kernel above).  `mean` is the plain sum over all samples / n and does not go through K.
// No atomics; 4-byte loads in (1), whose sums have an order to keep; (3) has none and moves 16 bytes per lane where aligned.
constexpr int RS_MAX_CHUNKS = STD_MAX_CHUNKS;          // slots of (2)'s merge tree
constexpr int RS_STATE_WORDS = 8;                      // n, mean - K, M2, K, sum, mean, sigma, scale

__device__ __forceinline__ StdMoments rs_shfl_down(const StdMoments a, const int off) {
    return StdMoments{__shfl_down(a.n, off, 64), __shfl_down(a.sum, off, 64), __shfl_down(a.mean, off, 64), __shfl_down(a.m2, off, 64)};
}

__global__ __launch_bounds__(256) void reward_scale_scan_kernel(const int64_t S, const int N, const int T, const int64_t E,
                                                                const float* __restrict__ r, const uint8_t* __restrict__ done_post,
                                                                const double gamma, double* __restrict__ carry,
                                                                const double* __restrict__ state, double* __restrict__ partial) {
    const double K = state[0] > 0.0 ? state[3] : (double)r[0];
    double cnt = 0.0, sum = 0.0, mean = 0.0, m2 = 0.0;             // Welford over this lane's samples (mean: of x - K)
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < S; s += stride) {
        const int64_t e = N > 0 ? s / N : s;
        double c = carry[s];
        for (int t0 = 0; t0 < T; t0 += 4) {
            float rv[4];
            uint8_t dv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {                          // the four steps' operands are requested before the first wait
                const int t = t0 + k < T ? t0 + k : T - 1;
                rv[k] = r[(int64_t)t * S + s];
                dv[k] = done_post[(int64_t)t * E + e];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t0 + k < T) {
                    c = gamma * c + (double)rv[k];
                    const double xk = c - K;
                    cnt += 1.0;
                    sum += c;
                    const double d = xk - mean;
                    mean += d / cnt;
                    m2 += d * (xk - mean);
                    if (dv[k]) c = 0.0;
                }
            }
        }
        carry[s] = c;
    }
    StdMoments a{cnt, sum, mean, m2};
    for (int off = 32; off > 0; off >>= 1) a = std_merge(a, rs_shfl_down(a, off));      // (lanes off the end of the wave: self, unused)
    __shared__ StdMoments sw[4];
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const StdMoments m = std_merge(std_merge(sw[0], sw[1]), std_merge(sw[2], sw[3]));
        double* p = partial + (int64_t)blockIdx.x * 4;
        p[0] = m.n; p[1] = m.sum; p[2] = m.mean; p[3] = m.m2;
    }
}

__global__ __launch_bounds__(256) void reward_scale_merge_kernel(const int C, const float* __restrict__ r, const double eps,
                                                                 const double* __restrict__ partial, double* __restrict__ state) {
    const int tid = threadIdx.x;
    __shared__ StdMoments sm[256];
    {
        StdMoments a{0.0, 0.0, 0.0, 0.0}, b{0.0, 0.0, 0.0, 0.0};
        if (tid < C) a = StdMoments{partial[tid * 4], partial[tid * 4 + 1], partial[tid * 4 + 2], partial[tid * 4 + 3]};
        if (tid + 256 < C)
            b = StdMoments{partial[(tid + 256) * 4], partial[(tid + 256) * 4 + 1], partial[(tid + 256) * 4 + 2], partial[(tid + 256) * 4 + 3]};
        sm[tid] = std_merge(a, b);
    }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sm[tid] = std_merge(sm[tid], sm[tid + off]);
        __syncthreads();
    }
    if (tid == 0) {
        const bool fresh = !(state[0] > 0.0);
        const double K = fresh ? (double)r[0] : state[3];
        const StdMoments prior = fresh ? StdMoments{0.0, 0.0, 0.0, 0.0} : StdMoments{state[0], state[4], state[1], state[2]};
        const StdMoments m = std_merge(prior, sm[0]);
        const double sigma = sqrt(m.m2 / m.n);
        state[0] = m.n; state[1] = m.mean; state[2] = m.m2; state[3] = K; state[4] = m.sum;
        state[5] = m.sum / m.n;
        state[6] = sigma;
        state[7] = sigma > 0.0 ? 1.0 / (sigma + eps) : 1.0;
    }
}

__global__ __launch_bounds__(256) void reward_scale_apply_kernel(const int64_t n, const float* __restrict__ r, const float clip,
                                                                 const double* __restrict__ state, float* __restrict__ out) {
    const double scale = state[7];
#define NMARL_RS(v, o) { float y_ = (float)((double)(v) * scale); if (clip > 0.f) y_ = y_ < -clip ? -clip : (y_ > clip ? clip : y_); o = y_; }
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0) {
        const int64_t n4 = n >> 2;
        const float4* r4 = reinterpret_cast<const float4*>(r);
        float4* o4 = reinterpret_cast<float4*>(out);
        for (int64_t i = i0; i < n4; i += stride) {
            const float4 v = r4[i];
            float4 o;
            NMARL_RS(v.x, o.x) NMARL_RS(v.y, o.y) NMARL_RS(v.z, o.z) NMARL_RS(v.w, o.w)
            o4[i] = o;
        }
        const int64_t i = (n4 << 2) + i0;
        if (i < n) NMARL_RS(r[i], out[i])
    } else {
        for (int64_t i = i0; i < n; i += stride) NMARL_RS(r[i], out[i])
    }
#undef NMARL_RS
}

constexpr int LOSS_MAXA = 8;

// One row's softmax, clamped log and entropy, A <= LOSS_MAXA probabilities in registers (lanes k >= A hold 0); lpa / pa: those of action a.
__device__ __forceinline__ void loss_row_softmax(const float* __restrict__ l, const int A, const int a, float (&p)[LOSS_MAXA],
                                                 float (&lp)[LOSS_MAXA], float& H, float& lpa, float& pa) {
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < LOSS_MAXA; ++k) {
        p[k] = k < A ? l[k] : -INFINITY;
        m = fmaxf(m, p[k]);
    }
    float z = 0.0f;
#pragma unroll
    for (int k = 0; k < LOSS_MAXA; ++k) {
        p[k] = k < A ? expf(p[k] - m) : 0.0f;
        z += p[k];
    }
    H = 0.0f; lpa = 0.0f; pa = 0.0f;
#pragma unroll
    for (int k = 0; k < LOSS_MAXA; ++k) {
        p[k] = p[k] / z;
        lp[k] = logf(fminf(fmaxf(p[k], 1e-10f), 1.0f));
        if (k < A) H -= p[k] * lp[k];
        if (k == a) { lpa = lp[k]; pa = p[k]; }
    }
}

// dl[k] = gn (d policy + d entropy) / d logit_k of a row, `w_pol` the weight of the policy term (ADV, or ADV rho gate of the surrogate):
//   g_k = dH/dpi_k = -(log_pi_k + c_k), c_k = [pi_k >= 1e-10];  dH/dlogit_j = pi_j (g_j - sum_k pi_k g_k)
__device__ __forceinline__ void loss_row_dlogits(const int A, const int a, const float (&p)[LOSS_MAXA], const float (&lp)[LOSS_MAXA],
                                                 const float pa, const float w_pol, const float e_coef, const float gn,
                                                 float* __restrict__ dl) {
    float gbar = 0.0f;
#pragma unroll
    for (int k = 0; k < LOSS_MAXA; ++k)
        if (k < A) gbar += p[k] * -(lp[k] + (p[k] >= 1e-10f ? 1.0f : 0.0f));
    const float ca = pa >= 1e-10f ? 1.0f : 0.0f;
#pragma unroll
    for (int k = 0; k < LOSS_MAXA; ++k)
        if (k < A) {
            const float gk = -(lp[k] + (p[k] >= 1e-10f ? 1.0f : 0.0f));
            const float d_pol = -w_pol * ca * ((k == a ? 1.0f : 0.0f) - p[k]);
            const float d_ent = -e_coef * p[k] * (gk - gbar);
            dl[k] = gn * (d_pol + d_ent);
        }
}

// The block's sums of NT per-thread partial columns, in a fixed order (lanes by shuffle, then the four waves as ((w0 + w1) + w2) + w3),
// to the block's slot of agent n's `partial` [N, gridDim.x, NT] (the index is formed inside the guarded store, by the NT lanes that write)
template <int NT>
__device__ __forceinline__ void loss_block_partials(float (&s)[NT], float* __restrict__ partial, const int n) {
    __shared__ float red[4][NT];
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NT; ++k) s[k] += __shfl_down(s[k], off, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NT; ++k) red[w][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < NT)
        partial[((int64_t)n * gridDim.x + blockIdx.x) * NT + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// A2C loss of Policy.prepare_loss (policies.py:20-30; NCMultiAgentPolicy 232-255) for all agents and rows:
//   pi = softmax(logits); log_pi = log(clip(pi, 1e-10, 1)); H = -sum pi log_pi
//   policy = -mean(log_pi[a] ADV);  value = 0.5 v_coef mean((R - v)^2);  entropy = -e_coef mean(H)
// fwd: per-block partial sums of the three terms -> loss_reduce_kernel<3> (fixed order).  bwd: the closed-form
// gradient w.r.t. logits and v (clip passes the gradient where 1e-10 <= pi), scaled by the per-agent upstream g.
// logits [N,rows,A] with row pitch l_row (a column block of the heads' GEMM output), everything else [N,rows];
// action [rows,N] u8.  One pass each instead of ~35 elementwise / reduction launches over [N,rows,A].
template <bool BWD>
__global__ __launch_bounds__(256) void a2c_loss_kernel(const int64_t rows, const int N, const int A, const int rows_per_block,
                                                       const float* __restrict__ logits, const int64_t l_sn, const int64_t l_row,
                                                       const float* __restrict__ v, const uint8_t* __restrict__ action,
                                                       const float* __restrict__ adv, const float* __restrict__ R,
                                                       const float v_coef, const float e_coef, const float* __restrict__ g_up,
                                                       float* __restrict__ partial, float* __restrict__ dlogits,
                                                       float* __restrict__ dv) {
    const int n = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    const float inv_m = 1.0f / (float)rows;
    const float gn = BWD ? g_up[n] * inv_m : 0.0f;
    float s[3] = {0.0f, 0.0f, 0.0f};                               // policy, value, entropy
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
        const int a = action[r * N + n];
        float p[LOSS_MAXA], lp[LOSS_MAXA], H, lpa, pa;
        loss_row_softmax(logits + (int64_t)n * l_sn + r * l_row, A, a, p, lp, H, lpa, pa);
        const int64_t i = (int64_t)n * rows + r;
        const float ad = adv[i], dR = R[i] - v[i];
        if (!BWD) {
            s[0] -= lpa * ad;
            s[1] += dR * dR;
            s[2] += H;
        } else {
            loss_row_dlogits(A, a, p, lp, pa, ad, e_coef, gn, dlogits + i * A);
            dv[i] = -gn * v_coef * dR;
        }
    }
    if (!BWD) loss_block_partials(s, partial, n);
}

// Second stage of a loss forward: column k of the C per-block partials of agent n in index order, / rows; column 1 (value) times
// 0.5 v_coef, column 2 (entropy) times -e_coef, every other column the plain mean.  NT = 3 (A2C), 5 (PPO), 6 (PPO with value clip).
template <int NT>
__global__ __launch_bounds__(64) void loss_reduce_kernel(const int C, const int64_t rows, const float v_coef, const float e_coef,
                                                         const float* __restrict__ partial, float* __restrict__ out /*[N,NT]*/) {
    const int n = blockIdx.x, k = threadIdx.x;
    if (k >= NT) return;
    float s = nmarl_ordered_sum(partial + (int64_t)n * C * NT + k, NT, C);
    s /= (float)rows;
    out[n * NT + k] = k == 1 ? s * 0.5f * v_coef : k == 2 ? -s * e_coef : s;
}

// logp_out[n, r] = log(clip(softmax(logits[n, r])[action[r, n]], 1e-10, 1)): one thread per row
__global__ __launch_bounds__(256) void ppo_logp_kernel(const int64_t rows, const int N, const int A, const float* __restrict__ logits,
                                                       const int64_t l_sn, const int64_t l_row, const uint8_t* __restrict__ action,
                                                       float* __restrict__ logp_out) {
    const int n = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float p[LOSS_MAXA], lp[LOSS_MAXA], H, lpa, pa;
    loss_row_softmax(logits + (int64_t)n * l_sn + r * l_row, A, action[r * N + n], p, lp, H, lpa, pa);
    logp_out[(int64_t)n * rows + r] = lpa;
}

// Opt-in PPO epochs (MODEL_CONFIG ppo_epochs > 1; the reference has none): the clipped surrogate against the behaviour policy's
// log-probabilities logp_old [N,rows], for epochs 2..K of an update.  The row arithmetic is the A2C loss's (loss_row_softmax,
// loss_row_dlogits), so that at logp_old = lp_a (rho = 1.0f exactly) the gradient has the bits of the A2C one.
//   rho = exp(lp_a - logp_old);  policy = -mean(min(rho ADV, clip(rho, 1-eps, 1+eps) ADV));  value, entropy: as above
//   approx_kl = mean((rho - 1) - (lp_a - logp_old));  clip_frac = mean(|rho - 1| > eps)
//   d policy / d logit_k = -ADV rho gate c_a (delta_ka - pi_k);  gate = 0 where (ADV > 0, rho > 1+eps) or (ADV < 0, rho < 1-eps)
// VCLIP (opt-in MODEL_CONFIG ppo_vclip): the PPO2 clipped value loss against v_old [N,rows], one more 4-byte load per row and a
// sixth partial column:
//   d = v - v_old;  inside = |d| <= vclip;  v_c = v_old + clip(d, -vclip, +vclip);  e1 = (R - v)^2;  e2 = (R - v_c)^2
//   e = inside ? e1 : max(e1, e2)  (inside is tested: v_old + (v - v_old) is not v in fp32);  value = 0.5 v_coef mean(e)
//   d value / d v = -v_coef (R - v) / rows where inside or e1 >= e2, else 0;  vclip_frac = mean(|d| > vclip)
template <bool BWD, bool VCLIP = false>
__global__ __launch_bounds__(256) void ppo_loss_kernel(const int64_t rows, const int N, const int A, const int rows_per_block,
                                                       const float* __restrict__ logits, const int64_t l_sn, const int64_t l_row,
                                                       const float* __restrict__ v, const uint8_t* __restrict__ action,
                                                       const float* __restrict__ adv, const float* __restrict__ R,
                                                       const float* __restrict__ logp_old, const float clip, const float v_coef,
                                                       const float e_coef, const float* __restrict__ g_up,
                                                       float* __restrict__ partial, float* __restrict__ dlogits,
                                                       float* __restrict__ dv, const float* __restrict__ v_old = nullptr,
                                                       const float vclip = 0.0f) {
    constexpr int NT = VCLIP ? 6 : 5;
    const int n = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    const float inv_m = 1.0f / (float)rows;
    const float gn = BWD ? g_up[n] * inv_m : 0.0f;
    const float lo_c = 1.0f - clip, hi_c = 1.0f + clip;
    float s[NT] = {};                                              // policy, value, entropy, approx_kl, clip_frac(, vclip_frac)
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
        const int a = action[r * N + n];
        float p[LOSS_MAXA], lp[LOSS_MAXA], H, lpa, pa;
        loss_row_softmax(logits + (int64_t)n * l_sn + r * l_row, A, a, p, lp, H, lpa, pa);
        const int64_t i = (int64_t)n * rows + r;
        const float ad = adv[i], dR = R[i] - v[i];
        const float dlp = lpa - logp_old[i];
        const float rho = expf(dlp);
        float e_v = 0.0f, over = 0.0f;
        bool v_open = true;
        if (VCLIP) {
            const float vo = v_old[i];
            const float d = v[i] - vo;
            const bool inside = fabsf(d) <= vclip;
            const float dRc = R[i] - (vo + fminf(fmaxf(d, -vclip), vclip));
            const float e1 = dR * dR, e2 = dRc * dRc;
            e_v = inside ? e1 : fmaxf(e1, e2);
            v_open = inside || e1 >= e2;
            over = fabsf(d) > vclip ? 1.0f : 0.0f;
        }
        if (!BWD) {
            s[0] -= fminf(rho * ad, fminf(fmaxf(rho, lo_c), hi_c) * ad);
            if (VCLIP) {
                s[1] += e_v;
                s[NT - 1] += over;
            } else {
                s[1] += dR * dR;
            }
            s[2] += H;
            // (rho - 1) - log rho >= 0; rho - 1 taken as expm1 of the difference: expf's rounding (6e-8) would swamp a term of d^2 / 2
            s[3] += fmaxf(expm1f(dlp) - dlp, 0.0f);
            s[4] += fabsf(rho - 1.0f) > clip ? 1.0f : 0.0f;
        } else {
            // the clipped branch is the smaller one, and constant in rho, exactly where the gate closes
            const bool closed = (ad > 0.0f && rho > hi_c) || (ad < 0.0f && rho < lo_c);
            loss_row_dlogits(A, a, p, lp, pa, ad * (closed ? 0.0f : rho), e_coef, gn, dlogits + i * A);   // rho = 1.0f: ad itself
            dv[i] = v_open ? -gn * v_coef * dR : 0.0f;
        }
    }
    if (!BWD) loss_block_partials(s, partial, n);
}

// Opt-in KL stop of the PPO epochs (MODEL_CONFIG ppo_target_kl), no host synchronisation.  gate: int32 x 4 owned by the model --
// [0] stop (what nmarl_rmsprop_tf_clip_guarded / nmarl_adam_clip_guarded take as their status word: while != 0 a step changes
// nothing), [1] the steps those refused, [2] ppo_epochs_done, [3] unused; the host resets it to (0, 0, 1, 0) at the start of every update.
//   ppo_kl_sum_kernel:  tail[0] = sum over agents of terms[n, 3] (approx_kl) in index order -- the float behind the gradient, so
//                       that the update's one all-reduce per epoch carries it and every rank sees the same sum
//   ppo_kl_gate_kernel: kl = tail[0] / count (count = ranks x agents);  kl > kappa (or NaN) raises stop, which stays raised;
//                       while stop is 0 the epoch counts as done
// One thread each: N <= a few dozen, and one owner of the words needs no atomics.
__global__ __launch_bounds__(64) void ppo_kl_sum_kernel(const int N, const float* __restrict__ terms, const int64_t t_stride,
                                                        float* __restrict__ tail) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float s = 0.0f;
    for (int n = 0; n < N; ++n) s += terms[(int64_t)n * t_stride + 3];
    tail[0] = s;
}

__global__ __launch_bounds__(64) void ppo_kl_gate_kernel(const float* __restrict__ tail, const int count, const float kappa,
                                                         int32_t* __restrict__ gate) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float kl = tail[0] / (float)count;
    int32_t stop = gate[0];
    if (!(kl <= kappa)) stop = 1;                 // strict: kl == kappa goes on; a NaN fails closed
    gate[0] = stop;
    if (stop == 0) gate[2] = gate[2] + 1;
}

inline int grid_x(int64_t n, int cap = 2048) {
    int64_t b = (n + 255) / 256;
    return (int)(b < cap ? (b > 0 ? b : 1) : cap);
}

}  // namespace

static bool strides_ok(int64_t E, int H, const int64_t* st4, int n4, const int64_t* st1, int n1) {
    for (int i = 0; i < n4; ++i) if (st4[i] < E * 4 * (int64_t)H || st4[i] % 4) return false;
    for (int i = 0; i < n1; ++i) if (st1[i] < E * (int64_t)H || st1[i] % 4) return false;
    return true;
}

extern "C" int nmarl_lstm_cell_fwd(int64_t E, int32_t N, int32_t H, const float* z, int64_t z_sn,
                                   const float* z2, int64_t z2_sn, const float* bias, int64_t bias_sn, const float* c_prev, int64_t c_prev_sn,
                                   const float* done, float* gates, int64_t gates_sn, float* c_new,
                                   int64_t c_new_sn, float* h_new, int64_t h_new_sn, void* stream) {
    if (E < 0 || N <= 0 || H <= 0 || H % 4 || bias_sn < 4 * (int64_t)H || bias_sn % 4 ||
        (E > 0 && (!z || !bias || !c_prev || !done || !c_new || !h_new)))
        return NMARL_EINVAL;
    const int64_t s4[3] = {z_sn, gates ? gates_sn : z_sn, z2 ? z2_sn : z_sn}, s1[3] = {c_prev_sn, c_new_sn, h_new_sn};
    if (!strides_ok(E, H, s4, 3, s1, 3)) return NMARL_EINVAL;
    if (E == 0) return NMARL_OK;
    CellStrides st{};
    st.z = z_sn; st.z2 = z2_sn; st.bias = bias_sn; st.c_prev = c_prev_sn; st.gates = gates_sn; st.c_new = c_new_sn; st.h_new = h_new_sn;
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(grid_x((int64_t)N * E * H / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), E, N, H, st, z, z2, bias, c_prev, done, gates, c_new, h_new);
    return nmarl_check_launch();
}

extern "C" int nmarl_lstm_cell_bwd(int64_t E, int32_t N, int32_t H, const float* gates, int64_t gates_sn,
                                   const float* c_prev, int64_t c_prev_sn, const float* c_new, int64_t c_new_sn,
                                   const float* done, const float* dh, int64_t dh_sn, const float* dh2,
                                   int64_t dh2_sn, const float* dc_new, int64_t dc_sn, float* dz, int64_t dz_sn,
                                   float* dc_prev, int64_t dc_prev_sn, void* stream) {
    if (E < 0 || N <= 0 || H <= 0 || H % 4 || (E > 0 && (!gates || !c_prev || !c_new || !done || !dz || !dc_prev)))
        return NMARL_EINVAL;
    const int64_t s4[2] = {gates_sn, dz_sn};
    const int64_t s1[6] = {c_prev_sn, c_new_sn, dc_prev_sn, dh ? dh_sn : c_new_sn, dc_new ? dc_sn : c_new_sn,
                           dh2 ? dh2_sn : c_new_sn};
    if (!strides_ok(E, H, s4, 2, s1, 6)) return NMARL_EINVAL;
    if (E == 0) return NMARL_OK;
    CellStrides st{};
    st.gates = gates_sn; st.c_prev = c_prev_sn; st.c_new = c_new_sn; st.dh = dh_sn; st.dh2 = dh2_sn; st.dc = dc_sn; st.dz = dz_sn;
    st.dc_prev = dc_prev_sn;
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(grid_x((int64_t)N * E * H / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), E, N, H, st, gates, c_prev, c_new, done, dh, dh2, dc_new, dz, dc_prev);
    return nmarl_check_launch();
}

extern "C" int nmarl_bias_act(int64_t rows, int32_t N, int32_t W, const float* x, int64_t x_sn, const float* bias,
                              int64_t bias_sn, int32_t act, float* y, int64_t y_sn, int64_t y_row, void* stream) {
    if (rows < 0 || N <= 0 || W <= 0 || W % 4 || act < 0 || act > 2 || x_sn < rows * W || x_sn % 4 || bias_sn < W ||
        bias_sn % 4 || y_row < W || y_row % 4 || y_sn < rows * y_row || y_sn % 4 || (rows > 0 && (!x || !bias || !y)))
        return NMARL_EINVAL;
    if (rows == 0) return NMARL_OK;
    hipLaunchKernelGGL(bias_act_kernel, dim3(grid_x((int64_t)N * rows * W / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), rows, N, W, x, x_sn, bias, bias_sn, act, y, y_sn, y_row);
    return nmarl_check_launch();
}

extern "C" int nmarl_sample_actions(int64_t E, int32_t N, int32_t A, const float* pi, const float* u, int32_t mode,
                                    uint64_t seed, int64_t env_id_base, int64_t step, const int64_t* step_dev,
                                    uint8_t* action, void* stream) {
    if (E < 0 || N <= 0 || A <= 0 || A > 255 || mode < 0 || mode > 2 || (E > 0 && (!pi || !action))) return NMARL_EINVAL;
    if (mode == 0 && E > 0 && !u) return NMARL_EINVAL;
    if (E == 0) return NMARL_OK;
    hipLaunchKernelGGL(sample_kernel, dim3(grid_x(E * N)), dim3(256), 0, static_cast<hipStream_t>(stream), E, N, A, pi,
                       u, mode, seed, env_id_base, step, step_dev, action);
    return nmarl_check_launch();
}

extern "C" int nmarl_nstep_return(int64_t E, int32_t N, int32_t T, const float* r, const float* v,
                                  const uint8_t* done_post, const float* R_end, double gamma, double alpha,
                                  const int32_t* dist, float* R_out, float* adv_out, void* stream) {
    if (E < 0 || N <= 0 || N > 64 || T <= 0 || (E > 0 && (!r || !v || !done_post || !R_end || !R_out || !adv_out)))
        return NMARL_EINVAL;
    if (alpha >= 0.0 && !dist) return NMARL_EINVAL;
    if (E == 0) return NMARL_OK;
    hipLaunchKernelGGL(nstep_kernel, dim3(grid_x((int64_t)N * E)), dim3(256), 0, static_cast<hipStream_t>(stream), E, N,
                       T, r, v, done_post, R_end, gamma, alpha, dist, R_out, adv_out);
    return nmarl_check_launch();
}

extern "C" int nmarl_gae_return(int64_t E, int32_t N, int32_t T, const float* r, const float* v, const uint8_t* done_post,
                                const float* R_end, double gamma, double lambda, double alpha, const int32_t* dist,
                                float* R_out, float* adv_out, void* stream) {
    if (E < 0 || N <= 0 || N > 64 || T <= 0 || (E > 0 && (!r || !v || !done_post || !R_end || !R_out || !adv_out)))
        return NMARL_EINVAL;
    if (alpha >= 0.0 && !dist) return NMARL_EINVAL;
    if (!(lambda >= 0.0 && lambda <= 1.0)) return NMARL_EINVAL;          // (NaN included)
    if (E == 0) return NMARL_OK;
    if (alpha >= 0.0)
        hipLaunchKernelGGL(gae_kernel<true>, dim3(grid_x((int64_t)N * E)), dim3(256), 0, static_cast<hipStream_t>(stream), E,
                           N, T, r, v, done_post, R_end, gamma, lambda, alpha, dist, R_out, adv_out);
    else
        hipLaunchKernelGGL(gae_kernel<false>, dim3(grid_x((int64_t)N * E)), dim3(256), 0, static_cast<hipStream_t>(stream), E,
                           N, T, r, v, done_post, R_end, gamma, lambda, alpha, dist, R_out, adv_out);
    return nmarl_check_launch();
}

extern "C" int nmarl_rmsprop_tf_clip_guarded(int32_t G, int64_t P, float* w, const float* g, float* ms, float* scratch,
                                             const float* lr_dev, float lr, float rho, float eps, float max_norm,
                                             float grad_scale, float* grad_norm_out, int32_t* status, void* stream) {
    if (G <= 0 || P <= 0 || !w || !g || !ms || !scratch || ((uintptr_t)status % 4)) return NMARL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sumsq_kernel, dim3(SUMSQ_BLOCKS, G), dim3(256), 0, s, P, g, scratch);
    hipLaunchKernelGGL(rmsprop_kernel, dim3(grid_x(P, 1024), G), dim3(256), 0, s, P, w, g, ms, scratch, lr_dev, lr, rho,
                       eps, max_norm, grad_scale, grad_norm_out, status);
    return nmarl_check_launch();
}

extern "C" int nmarl_rmsprop_tf_clip(int32_t G, int64_t P, float* w, const float* g, float* ms, float* scratch,
                                     const float* lr_dev, float lr, float rho, float eps, float max_norm,
                                     float grad_scale, float* grad_norm_out, void* stream) {
    return nmarl_rmsprop_tf_clip_guarded(G, P, w, g, ms, scratch, lr_dev, lr, rho, eps, max_norm, grad_scale, grad_norm_out,
                                         nullptr, stream);
}

extern "C" int nmarl_adam_clip_guarded(int32_t G, int64_t P, float* w, const float* g, float* m, float* v, float* scratch,
                                       int32_t* step, const float* lr_dev, float lr, float beta1, float beta2, float eps,
                                       float max_norm, float grad_scale, float* grad_norm_out, int32_t* status, void* stream) {
    if (G <= 0 || P < 0 || !w || !g || !m || !v || !scratch || !step || ((uintptr_t)step % 4) || ((uintptr_t)status % 4))
        return NMARL_EINVAL;
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps > 0.0f)) return NMARL_EINVAL;   // (NaN included)
    if (P == 0) return NMARL_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(adam_sumsq_kernel, dim3(SUMSQ_BLOCKS, G), dim3(256), 0, s, P, g, scratch, step, (const int32_t*)status);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_x(P, 1024), G), dim3(256), 0, s, P, w, g, m, v, scratch, (const int32_t*)step, lr_dev,
                       lr, beta1, beta2, eps, max_norm, grad_scale, grad_norm_out, status);
    return nmarl_check_launch();
}

extern "C" int nmarl_adam_clip(int32_t G, int64_t P, float* w, const float* g, float* m, float* v, float* scratch, int32_t* step,
                               const float* lr_dev, float lr, float beta1, float beta2, float eps, float max_norm,
                               float grad_scale, float* grad_norm_out, void* stream) {
    return nmarl_adam_clip_guarded(G, P, w, g, m, v, scratch, step, lr_dev, lr, beta1, beta2, eps, max_norm, grad_scale,
                                   grad_norm_out, nullptr, stream);
}

// Chunks per group of nmarl_standardize: G x chunks ~ 512 blocks, two per compute unit of a 256-CU device at G = 8 (64 chunks of
// 3840 rows at rows = 245 760) and at G = 1 (512 chunks of 6000 rows at rows = 3 072 000).  A function of the arguments alone (never
// of the device: two boxes cut and sum alike); it does not shrink for short groups -- chunks behind the last row are empty and merge
// as no-ops, so the launch shape of a captured graph follows G only.
extern "C" int nmarl_standardize_chunks(int64_t rows, int32_t G) {
    (void)rows;
    const int c = G > 0 ? (STD_MAX_CHUNKS + G - 1) / G : 1;
    return c < 1 ? 1 : (c > STD_MAX_CHUNKS ? STD_MAX_CHUNKS : c);
}

extern "C" int nmarl_standardize(int32_t G, int64_t rows, const float* x, int64_t x_sg, float* y, int64_t y_sg, double eps,
                                 double* partial, double* moments, void* stream) {
    if (rows < 1 || G < 0 || G > 65535 || x_sg < rows || y_sg < rows || !(eps >= 0.0)) return NMARL_EINVAL;   // (NaN included)
    if (G == 0) return NMARL_OK;
    if (!x || !y || !partial) return NMARL_EINVAL;
    const int C = nmarl_standardize_chunks(rows, G);
    const int64_t per = (rows + C - 1) / C;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(standardize_moments_kernel, dim3(C, G), dim3(256), 0, s, rows, per, x, x_sg, partial);
    hipLaunchKernelGGL(standardize_apply_kernel, dim3(C, G), dim3(256), 0, s, rows, per, x, x_sg, y, y_sg, eps,
                       (const double*)partial, moments);
    return nmarl_check_launch();
}

// Blocks of nmarl_reward_scale's scan, the first extent of its `partial`: one lane per stream up to RS_MAX_CHUNKS blocks (131 072
// streams), the streams behind that taken by the same lanes in a fixed grid-stride order.  A function of S alone, never of the device.
extern "C" int nmarl_reward_scale_chunks(int64_t S) {
    const int64_t c = (S + 255) / 256;
    return c < 1 ? 1 : (c > RS_MAX_CHUNKS ? RS_MAX_CHUNKS : (int)c);
}

extern "C" int nmarl_reward_scale(int64_t E, int32_t N_or_0, int32_t T, const float* r_raw, const uint8_t* done_post, double gamma,
                                  double eps, float clip, double* carry, double* state, double* partial, float* r_out, void* stream) {
    if (E < 1 || E > (1ll << 40) || N_or_0 < 0 || N_or_0 > 64 || T < 1 || !(eps >= 0.0) || !(gamma >= 0.0 && gamma <= 1.0) || clip != clip)
        return NMARL_EINVAL;                                                                                   // (NaN included)
    if (!r_raw || !done_post || !carry || !state || !partial || !r_out) return NMARL_EINVAL;
    const int64_t S = E * (N_or_0 > 0 ? N_or_0 : 1), n = S * T;
    const int C = nmarl_reward_scale_chunks(S);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(reward_scale_scan_kernel, dim3(C), dim3(256), 0, s, S, (int)N_or_0, (int)T, E, r_raw, done_post, gamma, carry,
                       (const double*)state, partial);
    hipLaunchKernelGGL(reward_scale_merge_kernel, dim3(1), dim3(256), 0, s, C, r_raw, eps, (const double*)partial, state);
    const int64_t blocks = (n / 4 + 255) / 256;
    hipLaunchKernelGGL(reward_scale_apply_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks))), dim3(256), 0, s, n,
                       r_raw, clip, (const double*)state, r_out);
    return nmarl_check_launch();
}

static int loss_chunks(int64_t rows, int N) {
    int64_t c = (rows * N + 4095) / 4096;            // ~16 rows per thread
    const int64_t cap = 2048 / (N > 0 ? N : 1) + 1;
    c = c > cap ? cap : c;
    return (int)(c < 1 ? 1 : c);
}

extern "C" int nmarl_a2c_loss_chunks(int64_t rows, int32_t N) { return rows > 0 && N > 0 ? loss_chunks(rows, N) : 0; }

static bool ppo_clip_ok(float clip) { return clip > 0.0f && clip <= 3.402823466e+38f; }      // (NaN fails both, inf the second)

enum LossKind { LOSS_A2C, LOSS_PPO, LOSS_PPO_VCLIP };

// The loss entries' one argument check and launch.  Forward: the loss kernel and its second stage (partial, loss_out must be there);
// backward: the loss kernel alone (g_up, dlogits, dv must be there).  logp_old / clip and v_old / vclip are checked for the kinds that read them.
static int loss_launch(LossKind kind, bool bwd, int64_t rows, int32_t N, int32_t A, const float* logits, int64_t l_sn, int64_t l_row,
                       const float* v, const uint8_t* action, const float* adv, const float* R, const float* logp_old,
                       const float* v_old, float clip, float vclip, float v_coef, float e_coef, const float* g_up, float* partial,
                       float* loss_out, float* dlogits, float* dv, void* stream) {
    if (rows <= 0 || N <= 0 || A <= 0 || A > LOSS_MAXA || l_row < A || !logits || !v || !action || !adv || !R) return NMARL_EINVAL;
    if (kind != LOSS_A2C && (!logp_old || !ppo_clip_ok(clip))) return NMARL_EINVAL;
    if (kind == LOSS_PPO_VCLIP && (!v_old || !ppo_clip_ok(vclip))) return NMARL_EINVAL;
    if (bwd ? (!g_up || !dlogits || !dv) : (!partial || !loss_out)) return NMARL_EINVAL;
    const int C = loss_chunks(rows, N);
    const int rpb = (int)((rows + C - 1) / C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (kind == LOSS_A2C) {
        const auto k = bwd ? a2c_loss_kernel<true> : a2c_loss_kernel<false>;
        hipLaunchKernelGGL(k, dim3(C, N), dim3(256), 0, st, rows, N, A, rpb, logits, l_sn, l_row, v, action, adv, R, v_coef, e_coef, g_up,
                           partial, dlogits, dv);
    } else {
        const auto k = kind == LOSS_PPO ? (bwd ? ppo_loss_kernel<true, false> : ppo_loss_kernel<false, false>)
                                        : (bwd ? ppo_loss_kernel<true, true> : ppo_loss_kernel<false, true>);
        hipLaunchKernelGGL(k, dim3(C, N), dim3(256), 0, st, rows, N, A, rpb, logits, l_sn, l_row, v, action, adv, R, logp_old, clip,
                           v_coef, e_coef, g_up, partial, dlogits, dv, v_old, vclip);
    }
    if (!bwd) {
        const auto k = kind == LOSS_A2C ? loss_reduce_kernel<3> : kind == LOSS_PPO ? loss_reduce_kernel<5> : loss_reduce_kernel<6>;
        hipLaunchKernelGGL(k, dim3(N), dim3(64), 0, st, C, rows, v_coef, e_coef, (const float*)partial, loss_out);
    }
    return nmarl_check_launch();
}

extern "C" int nmarl_a2c_loss_fwd(int64_t rows, int32_t N, int32_t A, const float* logits, int64_t l_sn, int64_t l_row,
                                  const float* v, const uint8_t* action, const float* adv, const float* R, float v_coef,
                                  float e_coef, float* partial, float* loss_out, void* stream) {
    return loss_launch(LOSS_A2C, false, rows, N, A, logits, l_sn, l_row, v, action, adv, R, nullptr, nullptr, 0.0f, 0.0f, v_coef, e_coef,
                       nullptr, partial, loss_out, nullptr, nullptr, stream);
}

extern "C" int nmarl_a2c_loss_bwd(int64_t rows, int32_t N, int32_t A, const float* logits, int64_t l_sn, int64_t l_row,
                                  const float* v, const uint8_t* action, const float* adv, const float* R, float v_coef,
                                  float e_coef, const float* g_up, float* dlogits, float* dv, void* stream) {
    return loss_launch(LOSS_A2C, true, rows, N, A, logits, l_sn, l_row, v, action, adv, R, nullptr, nullptr, 0.0f, 0.0f, v_coef, e_coef,
                       g_up, nullptr, nullptr, dlogits, dv, stream);
}

extern "C" int nmarl_ppo_logp(int64_t rows, int32_t N, int32_t A, const float* logits, int64_t l_sn, int64_t l_row,
                              const uint8_t* action, float* logp_out, void* stream) {
    if (rows <= 0 || N <= 0 || A <= 0 || A > LOSS_MAXA || l_row < A || !logits || !action || !logp_out) return NMARL_EINVAL;
    hipLaunchKernelGGL(ppo_logp_kernel, dim3((unsigned)((rows + 255) / 256), N), dim3(256), 0, static_cast<hipStream_t>(stream), rows,
                       N, A, logits, l_sn, l_row, action, logp_out);
    return nmarl_check_launch();
}

extern "C" int nmarl_ppo_loss_chunks(int64_t rows, int32_t N) { return nmarl_a2c_loss_chunks(rows, N); }

extern "C" int nmarl_ppo_loss_fwd(int64_t rows, int32_t N, int32_t A, const float* logits, int64_t l_sn, int64_t l_row,
                                  const float* v, const uint8_t* action, const float* adv, const float* R, const float* logp_old,
                                  float clip, float v_coef, float e_coef, float* partial, float* loss_out, void* stream) {
    return loss_launch(LOSS_PPO, false, rows, N, A, logits, l_sn, l_row, v, action, adv, R, logp_old, nullptr, clip, 0.0f, v_coef, e_coef,
                       nullptr, partial, loss_out, nullptr, nullptr, stream);
}

extern "C" int nmarl_ppo_loss_bwd(int64_t rows, int32_t N, int32_t A, const float* logits, int64_t l_sn, int64_t l_row,
                                  const float* v, const uint8_t* action, const float* adv, const float* R, const float* logp_old,
                                  float clip, float v_coef, float e_coef, const float* g_up, float* dlogits, float* dv,
                                  void* stream) {
    return loss_launch(LOSS_PPO, true, rows, N, A, logits, l_sn, l_row, v, action, adv, R, logp_old, nullptr, clip, 0.0f, v_coef, e_coef,
                       g_up, nullptr, nullptr, dlogits, dv, stream);
}

extern "C" int nmarl_ppo_loss_vclip_fwd(int64_t rows, int32_t N, int32_t A, const float* logits, int64_t l_sn, int64_t l_row,
                                        const float* v, const uint8_t* action, const float* adv, const float* R,
                                        const float* logp_old, const float* v_old, float clip, float vclip, float v_coef,
                                        float e_coef, float* partial, float* loss_out, void* stream) {
    return loss_launch(LOSS_PPO_VCLIP, false, rows, N, A, logits, l_sn, l_row, v, action, adv, R, logp_old, v_old, clip, vclip, v_coef,
                       e_coef, nullptr, partial, loss_out, nullptr, nullptr, stream);
}

extern "C" int nmarl_ppo_loss_vclip_bwd(int64_t rows, int32_t N, int32_t A, const float* logits, int64_t l_sn, int64_t l_row,
                                        const float* v, const uint8_t* action, const float* adv, const float* R,
                                        const float* logp_old, const float* v_old, float clip, float vclip, float v_coef,
                                        float e_coef, const float* g_up, float* dlogits, float* dv, void* stream) {
    return loss_launch(LOSS_PPO_VCLIP, true, rows, N, A, logits, l_sn, l_row, v, action, adv, R, logp_old, v_old, clip, vclip, v_coef,
                       e_coef, g_up, nullptr, nullptr, dlogits, dv, stream);
}

extern "C" int nmarl_ppo_kl_sum(int32_t N, const float* terms, int64_t t_stride, float* tail, void* stream) {
    if (N <= 0 || !terms || t_stride < 4 || !tail) return NMARL_EINVAL;
    hipLaunchKernelGGL(ppo_kl_sum_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), N, terms, t_stride, tail);
    return nmarl_check_launch();
}

extern "C" int nmarl_ppo_kl_gate(const float* tail, int32_t count, float kappa, int32_t* gate, void* stream) {
    if (!tail || count <= 0 || !ppo_clip_ok(kappa) || !gate || ((uintptr_t)gate % 4)) return NMARL_EINVAL;
    hipLaunchKernelGGL(ppo_kl_gate_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), tail, count, kappa, gate);
    return nmarl_check_launch();
}

extern "C" int nmarl_batch_epilogue(const nmarl_batch_epilogue_t* p, void* stream) {
    if (!p || p->E < 0 || p->N <= 0 || p->H <= 0 || p->A <= 0 || p->F <= 0 || p->T <= 0) return NMARL_EINVAL;
    if (p->E == 0) return NMARL_OK;
    if (!p->g || !p->done || !p->ep_sum || !p->ep_sq || !p->ep_len || !p->fin || !p->h_fw || !p->c_fw || !p->h_bw || !p->c_bw ||
        !p->fp_T || !p->fp_0 || !p->fp_uniform || !p->x_T || !p->x_0 || !p->done_pre)
        return NMARL_EINVAL;
    EpilogueArgs a{};
    a.E = p->E; a.N = p->N; a.H = p->H; a.A = p->A; a.F = p->F; a.T = p->T; a.T_env = p->T_env;
    a.g = p->g; a.done = p->done; a.ep_sum = p->ep_sum; a.ep_sq = p->ep_sq; a.ep_len = p->ep_len; a.fin = p->fin;
    a.h_fw = p->h_fw; a.c_fw = p->c_fw; a.h_bw = p->h_bw; a.c_bw = p->c_bw; a.fp_T = p->fp_T; a.fp_uniform = p->fp_uniform;
    a.x_T = p->x_T; a.fp_0 = p->fp_0; a.x_0 = p->x_0; a.done_pre = p->done_pre; a.skip_if = p->skip_if;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!p->scratch) return NMARL_EINVAL;
    int64_t sb = (a.E + EPI_BLOCK - 1) / EPI_BLOCK;
    sb = sb > EPI_MAX_BLOCKS ? EPI_MAX_BLOCKS : sb;
    hipLaunchKernelGGL(epilogue_stats_kernel, dim3((unsigned)sb), dim3(EPI_BLOCK), 0, st, a, p->scratch);
    const int64_t nh = (int64_t)a.N * a.E * a.H, nx = a.E * (int64_t)a.N * a.F;
    int64_t blocks = ((nh > nx ? nh : nx) + 255) / 256;
    blocks = blocks > 2048 ? 2048 : blocks;
    hipLaunchKernelGGL(epilogue_state_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, (const double*)p->scratch, (int)sb);
    return nmarl_check_launch();
}

// ---- several small device-to-device copies as ONE kernel launch.  Inside a captured hipGraph every launch of this library is a
// kernel node; aten's copy_ of a contiguous tensor is a hipMemcpyAsync, i.e. a memcpy node (the node class whose ordering
// against neighbouring kernel nodes round 5 found unreliable for memsets on this stack).
struct CopyMultiArgs {
    void* dst[NMARL_COPY_MAX];
    const void* src[NMARL_COPY_MAX];
    int64_t bytes[NMARL_COPY_MAX];
    const int32_t* skip_if;
};

__global__ void __launch_bounds__(256) copy_multi_kernel(const CopyMultiArgs a) {
    if (a.skip_if && *a.skip_if != 0) return;
    const int k = blockIdx.y;
    const int64_t n = a.bytes[k];
    char* __restrict__ d = static_cast<char*>(a.dst[k]);
    const char* __restrict__ s = static_cast<const char*>(a.src[k]);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    if (((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s)) & 15u) == 0) {
        const int64_t n16 = n >> 4;
        for (int64_t i = tid; i < n16; i += nth) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
        for (int64_t i = (n16 << 4) + tid; i < n; i += nth) d[i] = s[i];
    } else {
        for (int64_t i = tid; i < n; i += nth) d[i] = s[i];
    }
}

extern "C" int nmarl_copy_multi(int32_t n, void* const* dst, const void* const* src, const int64_t* bytes, const int32_t* skip_if,
                                void* stream) {
    if (n < 0 || n > NMARL_COPY_MAX || (n > 0 && (!dst || !src || !bytes))) return NMARL_EINVAL;
    if (n == 0) return NMARL_OK;
    CopyMultiArgs a{};
    a.skip_if = skip_if;
    int64_t most = 0;
    for (int k = 0; k < n; ++k) {
        if (bytes[k] < 0 || (bytes[k] > 0 && (!dst[k] || !src[k]))) return NMARL_EINVAL;
        a.dst[k] = dst[k]; a.src[k] = src[k]; a.bytes[k] = bytes[k];
        most = bytes[k] > most ? bytes[k] : most;
    }
    if (most == 0) return NMARL_OK;
    int64_t bx = (most / 16 + 255) / 256;                    // one 16-byte piece per thread, grid-stride above 1024 blocks
    bx = bx < 1 ? 1 : (bx > 1024 ? 1024 : bx);
    hipLaunchKernelGGL(copy_multi_kernel, dim3((unsigned)bx, (unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return nmarl_check_launch();
}

// ---- device time stamp: one thread stores the constant-rate wall clock (s_memrealtime: independent of the shader clock and of
// DVFS).  Measurement only (bench.py): two stamps around a launch inside a captured hipGraph give that launch's duration in its real
// neighbourhood, where event pairs cannot be placed and a with / without difference measures something else.
__global__ void timestamp_kernel(unsigned long long* out) { *out = wall_clock64(); }

extern "C" int nmarl_timestamp(uint64_t* out, void* stream) {
    if (!out) return NMARL_EINVAL;
    hipLaunchKernelGGL(timestamp_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), reinterpret_cast<unsigned long long*>(out));
    return nmarl_check_launch();
}

extern "C" int nmarl_timestamp_rate_khz(void) {
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return NMARL_EHIP;
    return khz;
}
