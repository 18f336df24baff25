// Synthetic (SUMO-free) ATSC grid for E lock-stepped replicas on gfx950: the reference's 5x5 lattice (nmarl_grid_step /
// nmarl_grid_reset, shape constants folded) and any rows x cols lattice of 2..32 intersections (nmarl_grid_step_rc /
// nmarl_grid_reset_rc: the same step body with the shape as uniform runtime values, csrc/grid_tile.h).
//
// Contract taken from the reference (envs/atsc_env.py:181-207 step, 216-240 yellow,
// 383-462 reward/state; envs/large_grid_env.py:23-27 phases, 58-105 topology;
// envs/large_grid_data/build_file.py:268-326 demand).  The dynamics are the
// store-and-forward model SPECIFIED in oracle/grid_ref.py (SUMO is not available,
// so the dynamics are "parity unpinned" w.r.t. the reference; the oracle is the spec).
//
// Mapping: one replica per 32-lane half wave, lane = intersection (25 of 32 lanes
// active), two replicas per wave64, 8 per 256-thread block.  A replica's state
// (q, transit: 2 x 25 x 6 fp32 = 1200 B, contiguous) is loaded with coalesced
// accesses into LDS; the neighbour exchange (desired link flows D, receiving space,
// spill-back scale) goes through LDS with wave barriers -- the 4-neighbourhood of the
// lattice never leaves the half wave.  Observation: COMPACT [25, 12] -- every node's OWN wave vector, what the reference
// hands an agent (atsc_env.py:253-262; 1200 contiguous bytes per replica, the batched engine's layout: the policy's
// encoder kernel gathers the neighbours itself) -- or the gathered slab [25, 5*12] (own + up to 4 neighbours in ascending
// node index, 6000 bytes) for the reference duck-type; assembled in LDS, 16-byte coalesced stores.
// HBM-bound (3.7 KB per replica-step with the compact observation, 8.5 KB with the slab); no MFMA.
// Any shape: lane = intersection for N = rows * cols <= 32 (lanes >= N add 0 to the reward butterfly and store nothing); all
// arrays dense in N ([E,N,6], [E,N,12 | 60]); 8 replicas x 6 N floats and 12 N / 60 N floats are multiples of 16 bytes for
// every N, so the block-wide 16-byte paths hold; LDS sized for 32 nodes (38 KB with the head-wait array).
#include "grid_tile.h"

namespace {

using namespace nmarl_grid;

// NT = 1: non-temporal stores for state and slab when the working set exceeds the caches (same effect as
// in csrc/cacc.hip: streaming writes at the fill ceiling instead of ~60 % of it).
// WAIT: the `wait` / `hybrid` objectives (atsc_env.py:383-418) -- one more state array, the head vehicle's waiting time per
// lane (oracle/grid_ref.py step 6); the shipped `queue` configs run the instantiation without it (same bytes as before).
template <int NT, bool COMPACT, bool WAIT>
__global__ __launch_bounds__(256) void grid_step_kernel(
    const nmarl_grid_params_t p, const int64_t E, const uint8_t* __restrict__ action,
    float* __restrict__ qs, float* __restrict__ trs, uint8_t* __restrict__ prev, int32_t* __restrict__ ts,
    float* __restrict__ xi, float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done,
    float* __restrict__ greward, const int auto_reset, const uint64_t seed, const int64_t env_id_base,
    int32_t* __restrict__ episode) {
    __shared__ __attribute__((aligned(16))) Lds lds[8];
    // state of the block's 8 replicas: 8 x 150 floats of q and of transit are CONTIGUOUS in memory (replica-major) and 16-byte
    // aligned (8 x 600 B per block step), so the whole block moves them with 16-byte accesses (300 float4 each way per array;
    // the 4-byte per-replica loops of rounds 1-3 were the kernel's issue limit in the HBM regime)
    __shared__ __attribute__((aligned(16))) float blk_q[8 * NQ], blk_tr[8 * NQ];
    __shared__ __attribute__((aligned(16))) float blk_w[WAIT ? 8 * NQ : 4];
    grid_step_groups<NT, COMPACT, WAIT, 8, false>(p, E, blockIdx.x, gridDim.x, action, nullptr, nullptr, 0u, qs, trs, prev, ts, xi, obs, reward, done,
                                                  greward, auto_reset, seed, env_id_base, episode, lds, blk_q, blk_tr, blk_w);
}

// the runtime-shape form: the same body (grid_tile.h, RT = true) on LDS sized for 32 nodes
template <int NT, bool COMPACT, bool WAIT>
__global__ __launch_bounds__(256) void grid_step_rc_kernel(
    const nmarl_grid_params_t p, const Shape<true> sh, const int64_t E, const uint8_t* __restrict__ action,
    float* __restrict__ qs, float* __restrict__ trs, uint8_t* __restrict__ prev, int32_t* __restrict__ ts,
    float* __restrict__ xi, float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done,
    float* __restrict__ greward, const int auto_reset, const uint64_t seed, const int64_t env_id_base,
    int32_t* __restrict__ episode) {
    __shared__ __attribute__((aligned(16))) LdsRc lds[8];
    __shared__ __attribute__((aligned(16))) float blk_q[8 * NQ_MAX], blk_tr[8 * NQ_MAX];
    __shared__ __attribute__((aligned(16))) float blk_w[WAIT ? 8 * NQ_MAX : 4];
    grid_step_groups<NT, COMPACT, WAIT, 8, false, true, LdsRc>(p, E, blockIdx.x, gridDim.x, action, nullptr, nullptr, 0u, qs, trs, prev, ts, xi, obs,
                                                               reward, done, greward, auto_reset, seed, env_id_base, episode, lds, blk_q,
                                                               blk_tr, blk_w, sh);
}

template <bool RT>
__device__ __forceinline__ void grid_reset_body(
    float* __restrict__ hws, const int64_t E, const uint8_t* __restrict__ mask, const float* __restrict__ u0, float* __restrict__ qs,
    float* __restrict__ trs, uint8_t* __restrict__ prev, int32_t* __restrict__ ts, float* __restrict__ xi,
    float* __restrict__ obs, const int obs_w, const uint64_t seed, const int64_t env_id_base, int32_t* __restrict__ episode,
    const Shape<RT> sh) {
    const int NN = sh.nn;
    const int l32 = threadIdx.x & 31;
    const int sub = threadIdx.x >> 5;
    for (int64_t e = (int64_t)blockIdx.x * 8 + sub; e < E; e += (int64_t)gridDim.x * 8) {
        if (mask != nullptr && mask[e] == 0) continue;
        for (int i = l32; i < NN * NLANE; i += 32) {
            qs[e * NN * NLANE + i] = 0.0f; trs[e * NN * NLANE + i] = 0.0f;
            if (hws) hws[e * NN * NLANE + i] = 0.0f;
        }
        for (int i = l32; i < NN * obs_w; i += 32) obs[e * NN * obs_w + i] = 0.0f;
        if (l32 < NN) prev[e * NN + l32] = 0;
        if (l32 == 0) ts[e] = 0;
        if (l32 < 4) {
            float U;
            if (u0 != nullptr) {
                U = u0[e * 4 + l32];
            } else {
                const Philox4 r4 = philox4x32_10((uint32_t)(env_id_base + e), 0u, (uint32_t)episode[e], NMARL_STREAM_RESET,
                                                 (uint32_t)seed, (uint32_t)(seed >> 32));
                const uint32_t w = l32 == 0 ? r4.x : l32 == 1 ? r4.y : l32 == 2 ? r4.z : r4.w;
                U = u01_from_bits(w);
            }
            xi[e * 4 + l32] = 0.8f + 0.4f * U;
        }
        __builtin_amdgcn_wave_barrier();
        if (u0 == nullptr && l32 == 4) episode[e] = episode[e] + 1;
    }
}

__global__ __launch_bounds__(256) void grid_reset_kernel(
    float* __restrict__ hws, const int64_t E, const uint8_t* __restrict__ mask, const float* __restrict__ u0, float* __restrict__ qs,
    float* __restrict__ trs, uint8_t* __restrict__ prev, int32_t* __restrict__ ts, float* __restrict__ xi,
    float* __restrict__ obs, const int obs_w, const uint64_t seed, const int64_t env_id_base, int32_t* __restrict__ episode) {
    grid_reset_body<false>(hws, E, mask, u0, qs, trs, prev, ts, xi, obs, obs_w, seed, env_id_base, episode, Shape<false>());
}

__global__ __launch_bounds__(256) void grid_reset_rc_kernel(
    float* __restrict__ hws, const int64_t E, const uint8_t* __restrict__ mask, const float* __restrict__ u0, float* __restrict__ qs,
    float* __restrict__ trs, uint8_t* __restrict__ prev, int32_t* __restrict__ ts, float* __restrict__ xi,
    float* __restrict__ obs, const int obs_w, const uint64_t seed, const int64_t env_id_base, int32_t* __restrict__ episode,
    const int nn) {
    grid_reset_body<true>(hws, E, mask, u0, qs, trs, prev, ts, xi, obs, obs_w, seed, env_id_base, episode, Shape<true>{0, 0, nn, 0});
}

inline int grid_blocks(int64_t E) {
    const int64_t b = (E + 7) / 8;
    return (int)(b < 4096 ? b : 4096);
}

// rows >= 1, cols >= 1, 2 <= rows * cols <= 32
inline bool grid_shape(int32_t rows, int32_t cols, Shape<true>& sh) {
    if (rows < 1 || cols < 1 || rows > NMAX || cols > NMAX || rows * cols < 2 || rows * cols > NMAX) return false;
    sh.rows = rows; sh.cols = cols; sh.nn = rows * cols; sh.inv_cols = (65536 + cols - 1) / cols;
    return true;
}

}  // namespace

extern "C" int nmarl_grid_step(const nmarl_grid_params_t* p, int64_t E, const uint8_t* action, float* q,
                               float* transit, uint8_t* prev_action, int32_t* t, float* xi, float* obs,
                               float* reward, uint8_t* done, float* global_reward, int32_t auto_reset,
                               uint64_t seed, int64_t env_id_base, int32_t* episode, void* stream) {
    if (!p || p->T <= 0 || p->norm_wave <= 0.f || E < 0 ||
        (E > 0 && (!action || !q || !transit || !prev_action || !t || !xi || !obs || !reward || !done || !global_reward)))
        return NMARL_EINVAL;
    if (auto_reset && !episode) return NMARL_EINVAL;
    if (p->objective < 0 || p->objective > 2 || (p->objective != 0 && E > 0 && !p->head_wait)) return NMARL_EINVAL;
    if (E == 0) return NMARL_OK;
    const bool nt = E * (p->compact_obs ? 4000 : 8800) > (int64_t)256 << 20;     // beyond the 256 MB Infinity Cache: stream the writes
    const bool wait = p->objective != 0;
#define NMARL_GRID_LAUNCH(NT_, C_, W_)                                                                                      \
    hipLaunchKernelGGL((grid_step_kernel<NT_, C_, W_>), dim3(grid_blocks(E)), dim3(256), 0, static_cast<hipStream_t>(stream), \
                       *p, E, action, q, transit, prev_action, t, xi, obs, reward, done, global_reward, auto_reset, seed,  \
                       env_id_base, episode)
#define NMARL_GRID_LAUNCH2(NT_, C_) { if (wait) NMARL_GRID_LAUNCH(NT_, C_, true); else NMARL_GRID_LAUNCH(NT_, C_, false); }
    if (p->compact_obs) { if (nt) NMARL_GRID_LAUNCH2(1, true) else NMARL_GRID_LAUNCH2(0, true) }
    else { if (nt) NMARL_GRID_LAUNCH2(1, false) else NMARL_GRID_LAUNCH2(0, false) }
#undef NMARL_GRID_LAUNCH2
#undef NMARL_GRID_LAUNCH
    return nmarl_check_launch();
}

extern "C" int nmarl_grid_reset(const nmarl_grid_params_t* p, int64_t E, const uint8_t* mask, const float* u0,
                                uint64_t seed, int64_t env_id_base, int32_t* episode, float* q, float* transit,
                                uint8_t* prev_action, int32_t* t, float* xi, float* obs, void* stream) {
    if (!p || E < 0 || (E > 0 && (!q || !transit || !prev_action || !t || !xi || !obs))) return NMARL_EINVAL;
    if (!u0 && !episode) return NMARL_EINVAL;
    if (E == 0) return NMARL_OK;
    hipLaunchKernelGGL(grid_reset_kernel, dim3(grid_blocks(E)), dim3(256), 0, static_cast<hipStream_t>(stream), p->head_wait, E, mask,
                       u0, q, transit, prev_action, t, xi, obs, p->compact_obs ? NL : OBSW, seed, env_id_base, episode);
    return nmarl_check_launch();
}

extern "C" int nmarl_grid_step_rc(const nmarl_grid_params_t* p, int64_t E, const uint8_t* action, float* q,
                                  float* transit, uint8_t* prev_action, int32_t* t, float* xi, float* obs,
                                  float* reward, uint8_t* done, float* global_reward, int32_t auto_reset,
                                  uint64_t seed, int64_t env_id_base, int32_t* episode, void* stream,
                                  int32_t rows, int32_t cols) {
    Shape<true> sh;
    if (!grid_shape(rows, cols, sh)) return NMARL_EINVAL;
    if (!p || p->T <= 0 || p->norm_wave <= 0.f || E < 0 ||
        (E > 0 && (!action || !q || !transit || !prev_action || !t || !xi || !obs || !reward || !done || !global_reward)))
        return NMARL_EINVAL;
    if (auto_reset && !episode) return NMARL_EINVAL;
    if (p->objective < 0 || p->objective > 2 || (p->objective != 0 && E > 0 && !p->head_wait)) return NMARL_EINVAL;
    if (E == 0) return NMARL_OK;
    // the 5x5 threshold (4000 / 8800 bytes per replica = 25 x 160 / 25 x 352) per node
    const bool nt = E * sh.nn * (p->compact_obs ? 160 : 352) > (int64_t)256 << 20;
    const bool wait = p->objective != 0;
#define NMARL_GRID_LAUNCH(NT_, C_, W_)                                                                                         \
    hipLaunchKernelGGL((grid_step_rc_kernel<NT_, C_, W_>), dim3(grid_blocks(E)), dim3(256), 0, static_cast<hipStream_t>(stream), \
                       *p, sh, E, action, q, transit, prev_action, t, xi, obs, reward, done, global_reward, auto_reset, seed, \
                       env_id_base, episode)
#define NMARL_GRID_LAUNCH2(NT_, C_) { if (wait) NMARL_GRID_LAUNCH(NT_, C_, true); else NMARL_GRID_LAUNCH(NT_, C_, false); }
    if (p->compact_obs) { if (nt) NMARL_GRID_LAUNCH2(1, true) else NMARL_GRID_LAUNCH2(0, true) }
    else { if (nt) NMARL_GRID_LAUNCH2(1, false) else NMARL_GRID_LAUNCH2(0, false) }
#undef NMARL_GRID_LAUNCH2
#undef NMARL_GRID_LAUNCH
    return nmarl_check_launch();
}

extern "C" int nmarl_grid_reset_rc(const nmarl_grid_params_t* p, int64_t E, const uint8_t* mask, const float* u0,
                                   uint64_t seed, int64_t env_id_base, int32_t* episode, float* q, float* transit,
                                   uint8_t* prev_action, int32_t* t, float* xi, float* obs, void* stream,
                                   int32_t rows, int32_t cols) {
    Shape<true> sh;
    if (!grid_shape(rows, cols, sh)) return NMARL_EINVAL;
    if (!p || E < 0 || (E > 0 && (!q || !transit || !prev_action || !t || !xi || !obs))) return NMARL_EINVAL;
    if (!u0 && !episode) return NMARL_EINVAL;
    if (E == 0) return NMARL_OK;
    hipLaunchKernelGGL(grid_reset_rc_kernel, dim3(grid_blocks(E)), dim3(256), 0, static_cast<hipStream_t>(stream), p->head_wait, E, mask,
                       u0, q, transit, prev_action, t, xi, obs, p->compact_obs ? NL : OBSW, seed, env_id_base, episode, sh.nn);
    return nmarl_check_launch();
}
