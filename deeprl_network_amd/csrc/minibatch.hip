// Replica minibatches of the opt-in PPO epochs (MODEL_CONFIG ppo_minibatches = M > 1): a permutation of the E replicas
// drawn on the device, and the gather that turns the strided rows of a group of E / M replicas into the dense tensors the update's
// forward pass, heads and loss read.  Kernel nodes only in a captured update; no atomics, no memset, no host synchronisation.
#include "common.h"

namespace {

constexpr int PERM_BLOCK = 256;

// key(e) = word x of Philox(e + env_id_base, epoch, count, NMARL_STREAM_MINIBATCH; seed): `count` (updates made so far) is read from
// the device, so a replayed graph draws a fresh permutation on every replay.
__global__ void __launch_bounds__(PERM_BLOCK) minibatch_keys_kernel(const int E, const uint64_t seed, const int64_t env_id_base,
                                                                     const int epoch, const int32_t* __restrict__ count,
                                                                     uint32_t* __restrict__ keys) {
    const int e = blockIdx.x * PERM_BLOCK + threadIdx.x;
    if (e >= E) return;
    const Philox4 r = philox4x32_10((uint32_t)(env_id_base + e), (uint32_t)epoch, (uint32_t)*count, NMARL_STREAM_MINIBATCH,
                                    (uint32_t)seed, (uint32_t)(seed >> 32));
    keys[e] = r.x;
}

// rank(e) = #{e' : (key(e'), e') < (key(e), e)}, perm[rank(e)] = e.  One thread per replica; the keys pass through LDS in tiles of
// PERM_BLOCK (every lane reads the same LDS word per step: a broadcast, no bank conflict).  E^2 compares: 16.8 M at E = 4096.
__global__ void __launch_bounds__(PERM_BLOCK) minibatch_rank_kernel(const int E, const uint32_t* __restrict__ keys,
                                                                     int32_t* __restrict__ perm) {
    __shared__ uint32_t tile[PERM_BLOCK];
    const int e = blockIdx.x * PERM_BLOCK + threadIdx.x;
    const uint32_t mine = e < E ? keys[e] : 0u;
    int rank = 0;
    for (int base = 0; base < E; base += PERM_BLOCK) {
        const int src = base + (int)threadIdx.x;
        tile[threadIdx.x] = src < E ? keys[src] : 0u;
        __syncthreads();
        const int n = E - base < PERM_BLOCK ? E - base : PERM_BLOCK;
        for (int i = 0; i < n; ++i) {
            const uint32_t k = tile[i];
            rank += (k < mine || (k == mine && base + i < e)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (e < E) perm[rank] = e;          // (rank < E: at most E - 1 pairs are smaller)
}

__global__ void minibatch_count_advance_kernel(int32_t* count) { *count = *count + 1; }

// ---- the gather: dst[o, i, :] = src[o, idx[i], :] for up to NMARL_GATHER_MAX (src, dst, outer, inner_bytes) descriptors in one launch
constexpr int GATHER_BLOCK = 256;
typedef uint32_t gather_u32x4 __attribute__((ext_vector_type(4)));     // (a native vector: HIP's uint4 array goes through scratch)
constexpr int GATHER_OPB = 8;            // outer slices one block takes with one idx read per thread (8 loads in flight, then 8 stores)

struct GatherOne {
    const char* src;
    char* dst;
    int64_t outer, inner;    // inner: bytes of one (o, e) row
    int64_t work;            // block work items = chunks * ceil(outer / GATHER_OPB)
    uint32_t upr, units;     // lanes per row (inner / width), lanes per outer slice (Em * upr)
    uint32_t chunks, width;  // ceil(units / GATHER_BLOCK); bytes one lane moves: 16, 4 or 1
};

struct GatherArgs {
    GatherOne d[NMARL_GATHER_MAX];
    const int32_t* idx;
    int32_t Em, E;
};

template <typename V>
__device__ __forceinline__ void gather_one(const GatherOne& d, const int32_t* __restrict__ idx, const int Em, const int E) {
    for (int64_t wk = blockIdx.x; wk < d.work; wk += gridDim.x) {
        const int64_t og = wk / d.chunks;
        const uint32_t q = (uint32_t)(wk - og * d.chunks) * GATHER_BLOCK + threadIdx.x;
        if (q >= d.units) continue;
        const uint32_t i = q / d.upr, u = q - i * d.upr;
        const int32_t e = idx[i];
        if (e < 0 || e >= E) continue;                      // an index outside [0, E): its destination row stays as it is
        const int64_t o0 = og * GATHER_OPB;
        const int64_t s_off = (int64_t)e * d.inner + (int64_t)u * sizeof(V), d_off = (int64_t)i * d.inner + (int64_t)u * sizeof(V);
        const int64_t s_o = (int64_t)E * d.inner, d_o = (int64_t)Em * d.inner;
        const char* __restrict__ s = d.src + o0 * s_o + s_off;
        char* __restrict__ t = d.dst + o0 * d_o + d_off;
        if (o0 + GATHER_OPB <= d.outer) {
            V v[GATHER_OPB];
#pragma unroll
            for (int k = 0; k < GATHER_OPB; ++k) v[k] = *reinterpret_cast<const V*>(s + k * s_o);
#pragma unroll
            for (int k = 0; k < GATHER_OPB; ++k) *reinterpret_cast<V*>(t + k * d_o) = v[k];
        } else {
            for (int64_t k = 0; o0 + k < d.outer; ++k) *reinterpret_cast<V*>(t + k * d_o) = *reinterpret_cast<const V*>(s + k * s_o);
        }
    }
}

__global__ void __launch_bounds__(GATHER_BLOCK) minibatch_gather_kernel(const GatherArgs a) {
    const GatherOne& d = a.d[blockIdx.y];
    if (d.width == 16) gather_one<gather_u32x4>(d, a.idx, a.Em, a.E);
    else if (d.width == 4) gather_one<uint32_t>(d, a.idx, a.Em, a.E);
    else gather_one<uint8_t>(d, a.idx, a.Em, a.E);
}

}  // namespace

extern "C" int nmarl_minibatch_perm(int32_t E, uint64_t seed, int64_t env_id_base, int32_t epoch, const int32_t* count_dev,
                                    uint32_t* keys_scratch, int32_t* perm_out, void* stream) {
    if (E < 1 || E > NMARL_MINIBATCH_MAX_E || !count_dev || !keys_scratch || !perm_out) return NMARL_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((E + PERM_BLOCK - 1) / PERM_BLOCK);
    hipLaunchKernelGGL(minibatch_keys_kernel, dim3(blocks), dim3(PERM_BLOCK), 0, st, E, seed, env_id_base, epoch, count_dev, keys_scratch);
    hipLaunchKernelGGL(minibatch_rank_kernel, dim3(blocks), dim3(PERM_BLOCK), 0, st, E, (const uint32_t*)keys_scratch, perm_out);
    return nmarl_check_launch();
}

extern "C" int nmarl_minibatch_count_advance(int32_t* count_dev, void* stream) {
    if (!count_dev) return NMARL_EINVAL;
    hipLaunchKernelGGL(minibatch_count_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), count_dev);
    return nmarl_check_launch();
}

extern "C" int nmarl_minibatch_gather(int32_t n, const nmarl_gather_desc_t* desc, const int32_t* idx, int32_t Em, int32_t E,
                                      void* stream) {
    if (n < 1 || n > NMARL_GATHER_MAX || Em < 1 || E < 1 || !desc || !idx) return NMARL_EINVAL;
    GatherArgs a{};
    a.idx = idx; a.Em = Em; a.E = E;
    int64_t most = 0;
    for (int k = 0; k < n; ++k) {
        const nmarl_gather_desc_t& s = desc[k];
        if (!s.src || !s.dst || s.outer < 1 || s.inner_bytes < 1) return NMARL_EINVAL;
        const uintptr_t bits = reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst) | (uintptr_t)s.inner_bytes;
        const uint32_t width = (bits & 15u) == 0 ? 16u : (bits & 3u) == 0 ? 4u : 1u;
        const int64_t upr = s.inner_bytes / width, units = upr * Em;
        if (units > (int64_t)1 << 31 || upr > (int64_t)1 << 31) return NMARL_EINVAL;      // (32-bit lane indices inside one outer slice)
        GatherOne& d = a.d[k];
        d.src = static_cast<const char*>(s.src); d.dst = static_cast<char*>(s.dst);
        d.outer = s.outer; d.inner = s.inner_bytes; d.width = width;
        d.upr = (uint32_t)upr; d.units = (uint32_t)units;
        d.chunks = (uint32_t)((units + GATHER_BLOCK - 1) / GATHER_BLOCK);
        d.work = (int64_t)d.chunks * ((s.outer + GATHER_OPB - 1) / GATHER_OPB);
        most = d.work > most ? d.work : most;
    }
    const int64_t bx = most > 4096 ? 4096 : most;           // grid-stride above 4096 blocks per descriptor
    hipLaunchKernelGGL(minibatch_gather_kernel, dim3((unsigned)bx, (unsigned)n), dim3(GATHER_BLOCK), 0,
                       static_cast<hipStream_t>(stream), a);
    return nmarl_check_launch();
}
