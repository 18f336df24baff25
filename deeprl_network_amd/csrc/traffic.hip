// Traffic record of an ATSC evaluation: the per-step row of the reference's `_traffic.csv` (envs/atsc_env.py:464-499,
// _measure_traffic_step) and the sums behind its `_trip.csv` (107-124), measured on the state the synthetic grid / network step
// kernels leave (csrc/grid.hip, csrc/realnet.hip; neither is touched: this kernel only READS q, transit, t, xi behind a step).
//
// SPECIFICATION (restated in float64 NumPy by tests/traffic_record_ref.py; parity unpinned like the dynamics: the
// reference measures individual SUMO vehicles, a fluid model has none).  "slot" = one of the N * S state entries of a replica
// (grid: S = 6 lanes per node; network: S = L links per node, the first n_s_i real).  Arithmetic in float64 on the float32 state.
//   static   mult[N][S]    detector entries of `ilds_in` that refer to the slot (grid 3,2,1,3,2,1; network 1 for k < n_s_i, else 0);
//                          a slot is valid where mult > 0;  M = sum mult
//            demand[4][12] veh/h of flow group g in 5-minute piece p (pieces >= 12: 0)
//   state    stand[N][S] f32 (s): how long the slot's queue has been standing without emptying;  prev_total f64;
//            cum[4] f64: sum departed, sum arrived, sum total * DT, sum halting * DT since `begin`
//   one call behind an env step WITHOUT auto-reset (q', transit', t' >= 1 are what the step left):
//     1. piece = ((t' - 1) * 5) / 300;  departed = sum_g demand[g][piece] / 3600 * DT * xi_g
//     2. halting = sum_valid q';  moving = sum_valid transit';  total = halting + moving
//     3. arrived = max(prev_total + departed - total, 0)      (both models conserve vehicles and never refuse an external arrival)
//     4. stand' = 0 if q' <= WAIT_EPS else stand + DT          (valid slots; the others stay 0)
//     5. avg_wait_sec = sum_valid q' * stand' / 2 / total      (0 if total <= WAIT_EPS)
//     6. avg_speed_mps = V_FREE * moving / total               (0 under the same condition)
//     7. avg_queue = sum mult * q' / M;  std_queue = sqrt(sum mult * (q' - avg_queue)^2 / M)       (np.std: population, two passes)
//     8. row, 8 x f32: number_total_car, number_departed_car, number_arrived_car, avg_wait_sec, avg_speed_mps, std_queue,
//        avg_queue, time_sec = 5 t';  then prev_total = total and cum advances.
//
// Mapping: one replica per wavefront, 4 replicas per 256-thread block, grid-stride over replicas.  The wave's 64 lanes stride over
// the replica's N * S <= 768 contiguous slots -- every load of q, transit, stand and every store of stand is coalesced -- and a lane
// keeps its <= 12 slots in registers, so the variance's second pass reads nothing again.  The partial sums are float64 and are
// reduced across the wave by an xor butterfly in a fixed order (IEEE addition commutes, so every lane ends with the same bits):
// results are bit-reproducible and do not depend on E or on the grid.  Lane 0 writes the row, prev_total and cum.  No LDS, no
// atomics, nothing crosses a wave.  Algorithmic bytes per replica: 16 N S (q, transit, stand in; stand out) + 4 N S (mult, from
// cache) + 120: 3.1 KB on the grid, 12.4 KB on Monaco.
#include "common.h"

namespace {

constexpr int NMAX = 32;          // nodes
constexpr int SMAX = 24;          // slots per node
constexpr int PER = NMAX * SMAX / NMARL_WAVE;      // slots a lane holds
constexpr int WAVES = 4;          // replicas per block
constexpr int N_GROUP = 4, N_PIECE = 12;
constexpr double DT = 5.0, V_FREE = 13.89, WAIT_EPS = 1e-3;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = NMARL_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, NMARL_WAVE);
    return v;
}

__global__ __launch_bounds__(NMARL_WAVE * WAVES) void traffic_step_kernel(
    const int64_t E, const int NS, const int32_t* __restrict__ mult, const double* __restrict__ demand,
    const float* __restrict__ qs, const float* __restrict__ trs, const int32_t* __restrict__ ts, const float* __restrict__ xi,
    float* __restrict__ stand, double* __restrict__ prev_total, double* __restrict__ cum, float* __restrict__ rec) {
    const int lane = threadIdx.x & (NMARL_WAVE - 1), wave = threadIdx.x / NMARL_WAVE;
    int m[PER];
    double msum = 0.0;
#pragma unroll
    for (int it = 0; it < PER; ++it) {
        const int i = it * NMARL_WAVE + lane;
        m[it] = i < NS ? mult[i] : 0;
        if (m[it] < 0) m[it] = 0;
        msum += (double)m[it];
    }
    const double M = wave_sum(msum);
    for (int64_t e = (int64_t)blockIdx.x * WAVES + wave; e < E; e += (int64_t)gridDim.x * WAVES) {
        float q[PER], tr[PER], st[PER];
#pragma unroll
        for (int it = 0; it < PER; ++it) {       // fixed trip count: all loads of the replica are in flight together
            const int i = it * NMARL_WAVE + lane;
            const bool in = i < NS;
            q[it] = in ? qs[e * NS + i] : 0.0f;
            tr[it] = in ? trs[e * NS + i] : 0.0f;
            st[it] = in ? stand[e * NS + i] : 0.0f;
        }
        double halting = 0.0, moving = 0.0, wq = 0.0, waited = 0.0;
#pragma unroll
        for (int it = 0; it < PER; ++it) {
            const int i = it * NMARL_WAVE + lane;
            const bool valid = m[it] > 0;
            const double qd = (double)q[it];
            st[it] = (valid && !(qd <= WAIT_EPS)) ? st[it] + (float)DT : 0.0f;
            if (valid) {
                halting += qd;
                moving += (double)tr[it];
                wq += (double)m[it] * qd;
                waited += qd * (double)st[it];
            }
            if (i < NS) stand[e * NS + i] = st[it];
        }
        halting = wave_sum(halting);
        moving = wave_sum(moving);
        wq = wave_sum(wq);
        waited = wave_sum(waited);
        const double avg_queue = M > 0.0 ? wq / M : 0.0;
        double var = 0.0;
#pragma unroll
        for (int it = 0; it < PER; ++it)
            if (m[it] > 0) {
                const double d = (double)q[it] - avg_queue;
                var += (double)m[it] * (d * d);
            }
        var = wave_sum(var);
        if (lane == 0) {
            const int t = ts[e];
            const int piece = t >= 1 ? ((t - 1) * 5) / 300 : N_PIECE;
            double departed = 0.0;
            if (piece < N_PIECE) {
#pragma unroll
                for (int g = 0; g < N_GROUP; ++g) departed += demand[g * N_PIECE + piece] / 3600.0 * DT * (double)xi[e * N_GROUP + g];
            }
            const double total = halting + moving;
            const double gone = prev_total[e] + departed - total;
            const double arrived = gone > 0.0 ? gone : 0.0;
            const bool some = total > WAIT_EPS;
            float* row = rec + e * 8;
            row[0] = (float)total;
            row[1] = (float)departed;
            row[2] = (float)arrived;
            row[3] = (float)(some ? waited / 2.0 / total : 0.0);
            row[4] = (float)(some ? V_FREE * moving / total : 0.0);
            row[5] = (float)(M > 0.0 ? sqrt(var / M) : 0.0);
            row[6] = (float)avg_queue;
            row[7] = (float)(5 * t);
            prev_total[e] = total;
            double* c = cum + e * 4;
            c[0] = c[0] + departed;
            c[1] = c[1] + arrived;
            c[2] = c[2] + total * DT;
            c[3] = c[3] + halting * DT;
        }
    }
}

__global__ __launch_bounds__(NMARL_WAVE * WAVES) void traffic_begin_kernel(
    const int64_t E, const int NS, const uint8_t* __restrict__ mask, float* __restrict__ stand, double* __restrict__ prev_total,
    double* __restrict__ cum) {
    const int lane = threadIdx.x & (NMARL_WAVE - 1), wave = threadIdx.x / NMARL_WAVE;
    for (int64_t e = (int64_t)blockIdx.x * WAVES + wave; e < E; e += (int64_t)gridDim.x * WAVES) {
        if (mask != nullptr && mask[e] == 0) continue;
        for (int i = lane; i < NS; i += NMARL_WAVE) stand[e * NS + i] = 0.0f;
        if (lane < 4) cum[e * 4 + lane] = 0.0;
        if (lane == 4) prev_total[e] = 0.0;
    }
}

inline int traffic_blocks(int64_t E) {
    const int64_t b = (E + WAVES - 1) / WAVES;
    return (int)(b < 4096 ? b : 4096);
}

inline bool sizes_ok(int64_t E, int32_t N, int32_t S) { return E >= 1 && N >= 1 && N <= NMAX && S >= 1 && S <= SMAX; }

}  // namespace

extern "C" int nmarl_atsc_traffic_begin(int64_t E, int32_t N, int32_t S, const uint8_t* mask, float* stand, double* prev_total,
                                        double* cum, void* stream) {
    if (!sizes_ok(E, N, S) || !stand || !prev_total || !cum) return NMARL_EINVAL;
    hipLaunchKernelGGL(traffic_begin_kernel, dim3(traffic_blocks(E)), dim3(NMARL_WAVE * WAVES), 0, static_cast<hipStream_t>(stream),
                       E, N * S, mask, stand, prev_total, cum);
    return nmarl_check_launch();
}

extern "C" int nmarl_atsc_traffic_step(int64_t E, int32_t N, int32_t S, const int32_t* mult, const double* demand, const float* q,
                                       const float* transit, const int32_t* t, const float* xi, float* stand, double* prev_total,
                                       double* cum, float* rec_row, void* stream) {
    if (!sizes_ok(E, N, S) || !mult || !demand || !q || !transit || !t || !xi || !stand || !prev_total || !cum || !rec_row)
        return NMARL_EINVAL;
    hipLaunchKernelGGL(traffic_step_kernel, dim3(traffic_blocks(E)), dim3(NMARL_WAVE * WAVES), 0, static_cast<hipStream_t>(stream),
                       E, N * S, mult, demand, q, transit, t, xi, stand, prev_total, cum, rec_row);
    return nmarl_check_launch();
}
