// The rule-based `maxpressure` agent of the ATSC scenarios (Varaiya 2013: per intersection the phase whose served movements hold
// the largest incoming-minus-downstream occupancy) for all E replicas in one launch.  It is the cross-node version of
// csrc/greedy.hip: the same (n_a, mask) table says which features of a node's own wave vector count for a phase, and every counted
// feature is first reduced by the mean occupancy of the links it discharges into -- other nodes' rows of the same replica.  ONE
// data-driven kernel serves the synthetic grid of any shape and the Monaco network: the scenario is the tables the host builds
// (envs/maxpressure.py grid_pressure_table, net_pressure_table).
//
// SPECIFICATION (restated in NumPy by tests/maxpressure_ref.py).  x[j][f] = (double) obs[e, j, f], feature f < F of
// node j's own wave vector; float64 throughout, every operation as written (the build has -ffp-contract=off):
//     occ_g      = (sum over the pairs p of group g, ascending from 0.0, of x[node_p][feat_p]) / (double) n_g
//     press(i,k) = x[i][k];  for r = 0, 1, 2 while tgrp[i][k][r] >= 0:  press = press - (double) tw[i][k][r] * occ[tgrp[i][k][r]]
//     score_a    = sum over the set bits k < F of mask[i][a], k ascending from 0.0, of press(i,k)
//     action[e,i]= the smallest a < n_a[i] with the largest score_a
// Observations are finite (the envs clip them).  The host has validated the tables (node < N, feature < F, group < G, n_g >= 1).
//
// Mapping: a block of 256 threads holds REPS = 4 replicas at a time and strides over the replicas by gridDim.x * REPS.
//   phase 0  thread = (replica, node, feature): the F leading floats of every row into LDS, 4-byte loads, consecutive lanes
//            consecutive floats of a row -- any row pitch and any alignment of the observation buffer are accepted as they are
//            (12 / 60 floats on the grid, 22 / 110 on the network: 110 floats are no multiple of 16 bytes), and only the own
//            vectors are fetched.  LDS rows have a pitch of 25 floats, so the 32 nodes of a replica fall on 32 different banks.
//   phase 1  thread = (replica, group): occ into LDS (<= 128 doubles per replica), the pairs as LDS offsets.
//   phase 2  thread = (replica, node), a replica's nodes in adjacent lanes: the pressure of every counted feature from the
//            node's own LDS row, its <= 3 terms and occ; eight float64 scores in registers; one byte stored per lane.
// Two __syncthreads() separate the phases, a third closes the iteration before the next replicas overwrite the rows.  The tables
// (<= 17 KB) are read once per block into LDS.  Every global address is formed from (replica, node < N, feature < F) alone --
// no table entry reaches one.  No atomics, no cross-block traffic: the result does not depend on E or on the launch grid.
// Phase 1 keeps four pairs' LDS reads in flight and phase 2 the three terms' (an absent term reads group 0 and is not applied);
// the adds and subtractions stay in the order of the specification.  68 VGPRs, 98 SGPRs, 33.9 KB LDS, no scratch
// (profiles/r17_maxpressure.txt).  Algorithmic bytes per replica-step: 4 N F in + N out = 1.2 KB on the 5x5 grid, 2.5 KB on Monaco.
#include "common.h"

namespace {

constexpr int NMAX = 32;          // nodes
constexpr int AMAX = 8;           // phases per node
constexpr int FMAX = 24;          // features of a node's own wave vector
constexpr int TMAX = 3;           // downstream terms per (node, feature)
constexpr int GMAX = 128;         // downstream groups
constexpr int PMAX = 768;         // (node, feature) pairs over all groups
constexpr int THREADS = 256;
constexpr int REPS = 4;           // replicas a block holds at a time
constexpr int XP = FMAX + 1;      // LDS pitch of a node's row, floats: odd, so adjacent nodes sit on different banks
constexpr int MAX_BLOCKS = 1024;

__global__ __launch_bounds__(THREADS) void atsc_maxpressure_kernel(
    const int64_t E, const int N, const int A_max, const int F, const int32_t* __restrict__ n_a, const uint32_t* __restrict__ mask,
    const int G, const int P, const int32_t* __restrict__ gptr, const int16_t* __restrict__ gpair,
    const int16_t* __restrict__ tgrp, const float* __restrict__ tw, const float* __restrict__ obs, const int64_t obs_row,
    uint8_t* __restrict__ action) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[NMAX * AMAX];
    __shared__ int s_na[NMAX];
    __shared__ int s_gptr[GMAX + 1];
    __shared__ uint16_t s_gpair[PMAX];                    // node * XP + feature: the pair's offset in a replica's rows
    __shared__ int16_t s_tgrp[NMAX * FMAX * TMAX];
    __shared__ float s_tw[NMAX * FMAX * TMAX];
    __shared__ float s_x[REPS][NMAX * XP];
    __shared__ double s_occ[REPS][GMAX];
    const int tid = threadIdx.x;
    // ---- the tables, once per block (visible behind the first barrier below)
    if (tid < N * AMAX) s_mask[tid] = mask[tid];
    if (tid < N) s_na[tid] = n_a[tid];
    if (tid <= G) s_gptr[tid] = gptr[tid];
    for (int p = tid; p < P; p += THREADS) s_gpair[p] = (uint16_t)((int)gpair[2 * p] * XP + (int)gpair[2 * p + 1]);
    for (int j = tid; j < N * FMAX * TMAX; j += THREADS) {
        s_tgrp[j] = tgrp[j];
        s_tw[j] = tw[j];
    }
    const int per = N * F;
    for (int64_t e0 = (int64_t)blockIdx.x * REPS; e0 < E; e0 += (int64_t)gridDim.x * REPS) {
        const int reps = E - e0 < REPS ? (int)(E - e0) : REPS;
        // ---- phase 0: the own vectors of `reps` replicas
        for (int idx = tid; idx < reps * per; idx += THREADS) {
            const int r = idx / per, rem = idx - r * per;
            const int i = rem / F, k = rem - i * F;
            s_x[r][i * XP + k] = obs[((e0 + r) * N + i) * obs_row + k];
        }
        __syncthreads();
        // ---- phase 1: the mean occupancy of every downstream group
        for (int idx = tid; idx < reps * G; idx += THREADS) {
            const int r = idx / G, g = idx - r * G;
            const int lo = s_gptr[g], hi = s_gptr[g + 1];
            double s = 0.0;
            for (int p = lo; p < hi; p += 4) {            // four pairs' LDS reads in flight; the adds stay in order
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = s_x[r][s_gpair[p + u < hi ? p + u : lo]];
#pragma unroll
                for (int u = 0; u < 4; ++u) s = p + u < hi ? s + (double)v[u] : s;
            }
            s_occ[r][g] = s / (double)(hi - lo);
        }
        __syncthreads();
        // ---- phase 2: scores and the first maximum
        for (int idx = tid; idx < reps * N; idx += THREADS) {
            const int r = idx / N, i = idx - r * N;
            const uint4 m_lo = *reinterpret_cast<const uint4*>(&s_mask[i * AMAX]);
            const uint4 m_hi = *reinterpret_cast<const uint4*>(&s_mask[i * AMAX + 4]);
            const uint32_t m[AMAX] = {m_lo.x, m_lo.y, m_lo.z, m_lo.w, m_hi.x, m_hi.y, m_hi.z, m_hi.w};
            uint32_t any = 0u;
#pragma unroll
            for (int a = 0; a < AMAX; ++a) any |= a < A_max ? m[a] : 0u;
            int na = s_na[i];
            na = na < 1 ? 1 : (na > A_max ? A_max : na);  // (the caller's contract is 1..A_max; nothing here indexes by it)
            double score[AMAX];
#pragma unroll
            for (int a = 0; a < AMAX; ++a) score[a] = 0.0;
#pragma unroll 2
            for (int k = 0; k < F; ++k) {
                if (!((any >> k) & 1u)) continue;         // no phase counts the feature
                double press = (double)s_x[r][i * XP + k];
                const int t0 = (i * FMAX + k) * TMAX;
                int g[TMAX];
                float w[TMAX];
                double o[TMAX];
#pragma unroll
                for (int t = 0; t < TMAX; ++t) {          // the three terms' reads are independent; an absent one reads group 0
                    g[t] = s_tgrp[t0 + t];
                    w[t] = s_tw[t0 + t];
                }
#pragma unroll
                for (int t = 0; t < TMAX; ++t) o[t] = s_occ[r][g[t] < 0 ? 0 : g[t]];
#pragma unroll
                for (int t = 0; t < TMAX; ++t) press = g[t] >= 0 ? press - (double)w[t] * o[t] : press;      // (left packed)
#pragma unroll
                for (int a = 0; a < AMAX; ++a) score[a] = ((m[a] >> k) & 1u) ? score[a] + press : score[a];
            }
            double best = score[0];
            int arg = 0;
#pragma unroll
            for (int a = 1; a < AMAX; ++a) {
                if (a < na && score[a] > best) {          // strictly greater: the first maximum stays
                    best = score[a];
                    arg = a;
                }
            }
            action[(e0 + r) * N + i] = (uint8_t)arg;
        }
        __syncthreads();                                  // the rows and occ are overwritten by the next iteration
    }
}

static_assert(NMAX * AMAX <= THREADS && GMAX + 1 <= THREADS, "mask and gptr are staged by one pass of the block");
static_assert(NMAX * XP <= 65535, "a pair's LDS offset is held in 16 bits");

}  // namespace

extern "C" int nmarl_atsc_maxpressure(int64_t E, int32_t N, int32_t A_max, int32_t F, const int32_t* n_a, const uint32_t* mask,
                                      int32_t G, int32_t P, const int32_t* gptr, const int16_t* gpair, const int16_t* tgrp,
                                      const float* tw, const float* obs, int64_t obs_row, uint8_t* action, void* stream) {
    if (E < 1 || N < 1 || N > NMAX || A_max < 1 || A_max > AMAX || F < 1 || F > FMAX) return NMARL_EINVAL;
    if (G < 0 || G > GMAX || P < 0 || P > PMAX || obs_row < F) return NMARL_EINVAL;
    if (!n_a || !mask || !gptr || !gpair || !tgrp || !tw || !obs || !action) return NMARL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(obs) & 3u) != 0) return NMARL_EINVAL;
    const int64_t want = (E + REPS - 1) / REPS;
    const dim3 grid((unsigned)(want < MAX_BLOCKS ? want : MAX_BLOCKS)), block(THREADS);
    hipLaunchKernelGGL(atsc_maxpressure_kernel, grid, block, 0, static_cast<hipStream_t>(stream), E, N, A_max, F, n_a, mask, G, P,
                       gptr, gpair, tgrp, tw, obs, obs_row, action);
    return nmarl_check_launch();
}
