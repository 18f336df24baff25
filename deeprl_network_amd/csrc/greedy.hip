// The rule-based `greedy` agent of the ATSC scenarios (reference: envs/large_grid_env.py:30-45 LargeGridController,
// envs/real_net_env.py:112-145 RealNetController) for all E replicas in one launch: per intersection the phase whose counted
// features of the node's own wave vector sum highest.  ONE data-driven kernel serves the synthetic grid of any shape and the
// Monaco network: the scenario is the table (n_a, mask) the host builds (envs/large_grid_env.py grid_greedy_table,
// envs/real_net_env.py net_greedy_table).  The network env's rows are 22 (1 + m_max) floats, no multiple of 4: its controller stages
// the own vectors into rows of 24 floats (envs/greedy.py).
//
// SPECIFICATION (restated in NumPy by the tests).  Node i of replica e, phase a < n_a[i]:
//     score_a     = sum of (double) obs_k over the set bits k of mask[i][a], k ascending from 0 (features 0..23)
//     action[e,i] = the smallest a with the largest score_a
// which is what the host controllers compute in float64 on the float32 observation (Python's `sum` / `q[a] + q[b]` add in
// ascending k, np.argmax returns the first maximum).  Bits at or above min(24, obs_row) refer to no feature of the node's own row
// and count nothing.  Observations are finite (the envs clip them).
//
// Mapping: thread = (replica, node), flat index g = e * N + i, so the nodes of a replica sit in adjacent lanes and a block's 256
// rows are one contiguous span of the observation buffer (N = 32: two replicas per wave, every lane a node).  A row is obs_row
// floats, a multiple of 4 (48 B compact grid, 240 B grid slab, 96 B for the network's staged own vectors), so a lane fetches its
// own <= 24 features with NV = min(6, obs_row / 4) 16-byte loads that are all issued before the first add (NV is a template
// parameter: the loads and
// the 24 x 8 predicated float64 adds are fully unrolled, features and scores stay in registers, no scratch).  The [N][8] mask
// table (<= 1 KB) and n_a are read once per block into LDS -- one dword per thread -- and a lane then reads its node's 8 words
// with two 16-byte LDS loads.  Phases at or above A_max are skipped by a wave-uniform branch.  The action is one byte per lane,
// adjacent lanes adjacent bytes.  No atomics, nothing crosses a lane: the result does not depend on E or on the launch grid.
// Algorithmic bytes per (replica, node): 16 NV in + 1 out = 49 (compact grid) / 97 (slab, network); per replica-step 1.2 KB on the
// 5x5 grid (compact), 2.7 KB on Monaco.
#include "common.h"

namespace {

constexpr int NMAX = 32;          // nodes
constexpr int AMAX = 8;           // phases per node
constexpr int FMAX = 24;          // features of a node's own wave vector
constexpr int THREADS = 256;

template <int NV>
__global__ __launch_bounds__(THREADS) void atsc_greedy_kernel(
    const int64_t rows, const int N, const int A_max, const int32_t* __restrict__ n_a, const uint32_t* __restrict__ mask,
    const float* __restrict__ obs, const int64_t obs_row, uint8_t* __restrict__ action) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[NMAX * AMAX];
    __shared__ int s_na[NMAX];
    const int tid = threadIdx.x;
    if (tid < N * AMAX) s_mask[tid] = mask[tid];          // N * 8 <= 256 = THREADS: the whole table in one pass
    if (tid < N) s_na[tid] = n_a[tid];
    __syncthreads();
    constexpr uint32_t LIVE = NV * 4 >= 32 ? 0xffffffffu : ((1u << (NV * 4)) - 1u);      // features the loaded row holds
    for (int64_t g = (int64_t)blockIdx.x * THREADS + tid; g < rows; g += (int64_t)gridDim.x * THREADS) {
        const int i = (int)(g % N);
        const float4* __restrict__ row = reinterpret_cast<const float4*>(obs + g * obs_row);
        float4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = row[j];       // fixed trip count: every load of the row is in flight together
        const uint4 m_lo = *reinterpret_cast<const uint4*>(&s_mask[i * AMAX]);
        const uint4 m_hi = *reinterpret_cast<const uint4*>(&s_mask[i * AMAX + 4]);
        const uint32_t m[AMAX] = {m_lo.x, m_lo.y, m_lo.z, m_lo.w, m_hi.x, m_hi.y, m_hi.z, m_hi.w};
        int na = s_na[i];
        na = na < 1 ? 1 : (na > A_max ? A_max : na);      // (the caller's contract is 1..A_max; nothing here indexes by it)
        double x[NV * 4];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            x[4 * j + 0] = (double)v[j].x;
            x[4 * j + 1] = (double)v[j].y;
            x[4 * j + 2] = (double)v[j].z;
            x[4 * j + 3] = (double)v[j].w;
        }
        double best = 0.0;
        int arg = 0;
#pragma unroll
        for (int a = 0; a < AMAX; ++a) {
            if (a < A_max) {                              // wave-uniform
                const uint32_t bits = m[a] & LIVE;
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < NV * 4; ++k) s = ((bits >> k) & 1u) ? s + x[k] : s;
                if (a == 0) {
                    best = s;
                } else if (a < na && s > best) {          // strictly greater: the first maximum stays
                    best = s;
                    arg = a;
                }
            }
        }
        action[g] = (uint8_t)arg;
    }
}

static_assert(NMAX * AMAX <= THREADS, "the mask table is staged by one pass of the block");

}  // namespace

extern "C" int nmarl_atsc_greedy(int64_t E, int32_t N, int32_t A_max, const int32_t* n_a, const uint32_t* mask, const float* obs,
                                 int64_t obs_row, uint8_t* action, void* stream) {
    if (E < 1 || N < 1 || N > NMAX || A_max < 1 || A_max > AMAX || !n_a || !mask || !obs || !action) return NMARL_EINVAL;
    if (obs_row < 4 || (obs_row & 3) != 0 || (reinterpret_cast<uintptr_t>(obs) & 15u) != 0) return NMARL_EINVAL;
    const int64_t rows = E * (int64_t)N;
    const int64_t want = (rows + THREADS - 1) / THREADS;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t nv = obs_row / 4 < FMAX / 4 ? obs_row / 4 : FMAX / 4;
#define NMARL_GREEDY_LAUNCH(NV) \
    hipLaunchKernelGGL(atsc_greedy_kernel<NV>, grid, block, 0, s, rows, N, A_max, n_a, mask, obs, obs_row, action)
    switch ((int)nv) {
        case 1: NMARL_GREEDY_LAUNCH(1); break;
        case 2: NMARL_GREEDY_LAUNCH(2); break;
        case 3: NMARL_GREEDY_LAUNCH(3); break;
        case 4: NMARL_GREEDY_LAUNCH(4); break;
        case 5: NMARL_GREEDY_LAUNCH(5); break;
        default: NMARL_GREEDY_LAUNCH(6); break;
    }
#undef NMARL_GREEDY_LAUNCH
    return nmarl_check_launch();
}
