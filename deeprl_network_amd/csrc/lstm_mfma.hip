// Fused LSTM step for agent-batched 64-unit cells on gfx950 matrix cores:
//
//     z = [x | h * (1 - done)] @ [Wx; Wh] (+ zadd1 + zadd2)      [rows x 256], fp32 MFMA
//     i,f,o = sigmoid(z + b), u = tanh(z + b);  c' = f * (c * (1 - done)) + i * u;  h' = o * tanh(c')
//
// i.e. agents/utils.py:102-113 (lstm), 199-208 (lstm_comm), 401-408 (lstm_ic3) with the cell fused into the GEMM
// epilogue: the [rows x 256] pre-activation never goes to HBM (the separate GEMM + cell pair writes and re-reads it:
// 2 x 33.5 MB per step at E = 4096).
//
// One kernel, lstm_step_x_kernel: K = KX + 64.  KX = 0 is the recurrent product alone (the x-side pre-activation, if
// any, arrives as an addend).  fp32 MFMA = the fp32 vector rate (157 TFLOP/s chip peak, MI355X_MICROARCH.md).
#include "common.h"
#include "cacc_tile.h"
#include "grid_tile.h"
#include <stdlib.h>
#include <type_traits>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int H = 64;
constexpr int G4 = 4 * H;          // 256 gate columns
constexpr int ROWS_B = 128;        // rows per block
constexpr int APITCH = H + 1;      // 65

struct FusedArgs {
    const float *h_in, *bias, *zadd1, *zadd2, *c_prev, *done;
    float *gates, *c_new, *h_new;
    int64_t h_sn, bias_sn, zadd1_sn, zadd2_sn, c_prev_sn, gates_sn, c_new_sn, h_new_sn;
    int64_t E;
    int blocks_per_agent;
    nmarl_head_t hd;               // actor / critic head of the epilogue (kind 0: none)
};

constexpr int MAXA = 8;            // widest action set the head epilogue keeps in registers

// Epilogue transcendentals: 160 per lane with ONE wave per SIMD, so their latency is fully exposed.
// sigmoid(x) = rcp(1 + 2^(-x log2 e)) on the hardware exp2 / rcp units (about 1 ulp each, relative error of the
// result <= ~1e-6 for |x| < 20; both saturate correctly), tanh(x) = 2 sigmoid(2x) - 1 (absolute error <= 2.4e-7).
// The separate cell kernel (other H, backward checks) keeps libm's expf / tanhf; both agree within 1e-6.
__device__ __forceinline__ float sigm(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float tanh_fast(float x) { return 2.0f * sigm(2.0f * x) - 1.0f; }

// ---------------------------------------------------------------------------------------------------------
// 16-row wave strips on v_mfma_f32_16x16x4_f32.  C/D layout of 16x16x4: col = lane & 15, row = 4 (lane >> 4) + reg ->
// the four gates of unit j = 16 jj + col are acc[jj], acc[4 + jj], acc[8 + jj], acc[12 + jj] at the same reg: the cell
// stays lane-local.
typedef float f32x4 __attribute__((ext_vector_type(4)));
// The same activations on the four rows a lane holds of one unit, written as vector arithmetic: operation for operation the scalar
// formulas above (packing changes no rounding), but the multiplies / adds around the transcendentals become packed fp32
// instructions (v_pk_mul_f32 / v_pk_add_f32: two values per issue slot -- the epilogues are issue-bound next to the MFMAs)
__device__ __forceinline__ f32x4 sigm4(const f32x4 x) {
    f32x4 t = x * -1.4426950408889634f;
    t[0] = __builtin_amdgcn_exp2f(t[0]); t[1] = __builtin_amdgcn_exp2f(t[1]);
    t[2] = __builtin_amdgcn_exp2f(t[2]); t[3] = __builtin_amdgcn_exp2f(t[3]);
    t = t + 1.0f;
    t[0] = __builtin_amdgcn_rcpf(t[0]); t[1] = __builtin_amdgcn_rcpf(t[1]);
    t[2] = __builtin_amdgcn_rcpf(t[2]); t[3] = __builtin_amdgcn_rcpf(t[3]);
    return t;
}
__device__ __forceinline__ f32x4 tanh4(const f32x4 x) { return sigm4(x * 2.0f) * 2.0f - 1.0f; }
constexpr int R16 = 16;                 // rows per wave
constexpr int WAVES2 = 8;

#ifdef NMARL_STEP_TIMELINE      // instrumentation build (tools/step_timeline.py): shader-clock stamps of block 0's waves
__device__ unsigned long long* g_timeline = nullptr;
__global__ void timeline_set_kernel(unsigned long long* p) { g_timeline = p; }
#define NMARL_STAMP(i) if (g_timeline && blockIdx.x == 0 && (threadIdx.x & 63) == 0) g_timeline[(threadIdx.x >> 6) * 64 + (i)] = __builtin_amdgcn_s_memtime();
#define NMARL_NOTE(i, v) if (g_timeline && blockIdx.x == 0 && (threadIdx.x & 63) == 0) g_timeline[(threadIdx.x >> 6) * 64 + (i)] = (unsigned long long)(v);
#else
#define NMARL_STAMP(i)
#define NMARL_NOTE(i, v)
#endif

// Critic head epilogue of one wave: its 16 fresh rows of h' sit in the wave's (now idle) LDS tile, the first 64 rows of
// the critic's weights in LDS (w_h, staged by the kernel).  Lane (row = lane & 15, quarter = lane >> 4) accumulates the
// quarter's 16 k, two xor-shuffles finish the 64-long dot; lanes 0..15 then own one row each: the value, plus (kind 2)
// the one-hot rows gathered from the neighbours' action bytes.
template <int KIND>
__device__ __forceinline__ void head_epilogue(const FusedArgs& a, const int n, const int N, const int64_t row0,
                                              const int lane, const float* a_tile, const float* w_h) {
    static_assert(KIND == 2 || KIND == 3, "critic heads only (the actor's is head_policy_lds)");
    const nmarl_head_t& hd = a.hd;
    const int rl = lane & 15, q = lane >> 4;
    float acc = 0.0f;
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
        const int k = q * 16 + kk;
        acc += a_tile[rl * APITCH + k] * w_h[k];
    }
    if (KIND == 3) { NMARL_STAMP(34) }
    acc += __shfl_xor(acc, 16, 64);
    acc += __shfl_xor(acc, 32, 64);
    if (KIND == 3) { NMARL_STAMP(35) }
    const int64_t row = row0 + rl;
    if (q != 0 || row >= a.E) return;
    const float* b = KIND == 3 ? hd.b2 + (int64_t)n * hd.b2_sn : hd.b + (int64_t)n * hd.b_sn;
    float v = acc + b[0];
    if (KIND == 2) {                    // kind 3 leaves the neighbour-action term to nmarl_nbr_action_value_fwd (the
        const float* w = hd.w + (int64_t)n * hd.w_sn;     // other agents' draws of this lock-step are made by other blocks)
        for (int k = 0; k < hd.m_max; ++k) {
            const int j = hd.nbr_idx[n * hd.m_max + k];
            if (j >= 0) v += w[H + k * hd.A + (int)hd.act_in[row * N + j]];
        }
    }
    hd.v_out[(int64_t)n * hd.v_sn + row] = v;
}

// Actor head + draw: weights / bias come zero-padded to MAXA columns from LDS (wl [64][MAXA], bl [MAXA]), so every loop
// runs over MAXA without a branch (padded logits are -inf -> probability exactly 0: adding them to the CDF sums is exact,
// and cum / tot = 1 <= u never holds for u < 1): a branchy version over A columns spent ~13 k cycles per wave here.  Same
// arithmetic as nmarl_draw_action otherwise.
// MA = columns actually processed: 8 (MAXA), or 4 when the net has at most 4 actions (CACC: A = 4) -- the padded columns carry
// logit -inf -> probability exactly 0 and add exact zeros to every sum, so leaving them out changes no bit; it halves the dot
// products, the exps, the divisions and the float64 CDF of the head (~570 -> ~300 vector instructions per wave, which only 16 of
// the 64 lanes need but every wave pays for in full).
// AN = columns that go through the softmax and the float64 CDF (A <= AN <= MA; the dot products and shuffles keep the float4 shape MA):
// the grid's five actions pay five exponentials / divisions / float64 CDF steps instead of eight -- dropped columns hold exact zeros
template <int MA, int AN = MA>
__device__ __forceinline__ int head_policy_lds_n(const FusedArgs& a, const int n, const int N, const int64_t row0,
                                                 const int lane, const float* a_tile, const float* wl, const float* bl) {
    static_assert(MAXA == 8 && (MA == 4 || MA == 8) && AN <= MA, "one or two float4 per k");
    const nmarl_head_t& hd = a.hd;
    const int A = hd.A;
    const int rl = lane & 15, q = lane >> 4;
    const int64_t row = row0 + rl;
    const int64_t rowc = row < a.E ? row : a.E - 1;
    // late inputs first: their latency hides behind the dot products
    const int64_t step = hd.step + (hd.step_dev ? *hd.step_dev : 0);
    const float uh = hd.mode == 0 ? hd.u[rowc * N + n] : 0.0f;
    float acc[MA];
#pragma unroll
    for (int o = 0; o < MA; ++o) acc[o] = 0.0f;
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
        const int k = q * 16 + kk;
        const float hk = a_tile[rl * APITCH + k];
        const float4 w0 = *reinterpret_cast<const float4*>(wl + k * MAXA);
        acc[0] += hk * w0.x; acc[1] += hk * w0.y; acc[2] += hk * w0.z; acc[3] += hk * w0.w;
        if (MA == 8) {
            const float4 w1 = *reinterpret_cast<const float4*>(wl + k * MAXA + 4);
            acc[MA - 4] += hk * w1.x; acc[MA - 3] += hk * w1.y; acc[MA - 2] += hk * w1.z; acc[MA - 1] += hk * w1.w;
        }
    }
#pragma unroll
    for (int o = 0; o < AN; ++o) {
        acc[o] += __shfl_xor(acc[o], 16, 64);
        acc[o] += __shfl_xor(acc[o], 32, 64);
    }
    if (q != 0 || row >= a.E) return -1;
    float p[AN];
    float m = -INFINITY;
#pragma unroll
    for (int o = 0; o < AN; ++o) {
        p[o] = o < A ? acc[o] + bl[o] : -INFINITY;
        m = fmaxf(m, p[o]);
    }
    float ssum = 0.0f;
#pragma unroll
    for (int o = 0; o < AN; ++o) {
        p[o] = expf(p[o] - m);                       // exp(-inf) = 0 for the padded columns
        ssum += p[o];
    }
#pragma unroll
    for (int o = 0; o < AN; ++o) p[o] = p[o] / ssum;
    float* po = hd.pi_out + (int64_t)n * hd.pi_sn + row * A;
    if (A == 4) {
        *reinterpret_cast<float4*>(po) = float4{p[0], p[1], p[2], p[3]};
    } else {
        for (int o = 0; o < A; ++o) po[o] = p[o];
    }
    int act = 0;
    if (hd.mode == 2) {
        float best = p[0];
#pragma unroll
        for (int k = 1; k < AN; ++k) {
            const bool gt = k < A && p[k] > best;
            best = gt ? p[k] : best;
            act = gt ? k : act;
        }
    } else {
        float uu = uh;
        if (hd.mode == 1) {
            const Philox4 r = philox4x32_10((uint32_t)(hd.env_id_base + row), (uint32_t)(n >> 2), (uint32_t)step, NMARL_STREAM_ACTION,
                                            (uint32_t)hd.seed, (uint32_t)(hd.seed >> 32));
            const uint32_t w = (n & 3) == 0 ? r.x : (n & 3) == 1 ? r.y : (n & 3) == 2 ? r.z : r.w;
            uu = u01_from_bits(w);
        }
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < AN; ++k) tot += (double)p[k];
        double cum = 0.0;
#pragma unroll
        for (int k = 0; k < AN; ++k) {
            cum += (double)p[k];
            act = (k < A && cum / tot <= (double)uu) ? k + 1 : act;
        }
        act = act > A - 1 ? A - 1 : act;
    }
    hd.act_out[row * N + n] = (uint8_t)act;
    return act;
}

// -> the action this lane drew for its row (lanes 0..15 of the wave, rows inside the batch), -1 elsewhere
__device__ __forceinline__ int head_policy_lds(const FusedArgs& a, const int n, const int N, const int64_t row0,
                                               const int lane, const float* a_tile, const float* wl, const float* bl) {
    if (a.hd.A <= 4) return head_policy_lds_n<4>(a, n, N, row0, lane, a_tile, wl, bl);       // (uniform)
    if (a.hd.A == 5) return head_policy_lds_n<8, 5>(a, n, N, row0, lane, a_tile, wl, bl);     // (the ATSC grid's five phases)
    return head_policy_lds_n<8>(a, n, N, row0, lane, a_tile, wl, bl);
}

// ---------------------------------------------------------------------------------------------------------
// lstm_step_x_kernel: the WHOLE pre-activation on the matrix cores,
//     z = [x | h * (1 - done)] @ [Wx; Wh] + bias (+ zadd1 + zadd2),   K = KX + 64  (KX = 0, 32, ... , 256)
// then the cell and the head epilogues above.  agents/utils.py:102-113 (lstm: x = fc output, KX = n_fc, or the
// [fcs | fcp] concatenation of policies.py:176-181, KX = 2 n_fc), :199-208 (lstm_comm: x = [hx | hp | hm], KX = 3 H),
// :401-408 (lstm_ic3: x = s, KX = H).  The separate library GEMM s @ Wx (25.6 us and 33.5 MB written + re-read per
// lock-step at E = 4096) disappears; what is left is bound by the fp32 matrix pipe.  KX = 0: the image holds Wh alone
// and whatever else the pre-activation has arrives as zadd1 / zadd2.
//
// Weights: [Wx; Wh] of an agent is (KX + 64) x 256 floats = up to 320 KB -- more than the 160 KB LDS -- so it streams
// through LDS in chunks of 32 k-rows, double buffered, from a pre-permuted IMAGE (nmarl_lstm_wimage, rebuilt once per
// weight update): chunk = [k][c = column & 15][t = column >> 4, padded to 20] floats = 40 KB, staged by plain
// 16-byte copies; a lane fetches the B operands of all 16 column tiles of one k with four conflict-free
// ds_read_b128.  The two Wh chunks come last, so after the K loop both LDS buffers still hold Wh: the value
// re-step of head kind 3 (quirk Q1) needs no re-staging.
// Activations: a wave owns 16 rows x all 256 columns (64 accumulator registers); its A operands are loaded from
// global memory straight into registers as float4 (lane (row = lane & 15, g = lane >> 4) takes k = 32 ch + 16 j + 4 g
// + {0..3}: 64-byte segments), one chunk ahead.  The MFMA k order inside a chunk is permuted accordingly -- A and B
// use the same permutation, so the product is unchanged.
// Block = 512 threads = 8 waves x 16 rows = 128 rows of agent (blockIdx % N): with N = 8 all blocks of an agent share
// an XCD, whose L2 then holds just that agent's image.  One barrier per chunk.
constexpr int CH_K = 32;                        // k rows per W chunk
constexpr int CH_FLOATS = CH_K * 16 * 20;       // 10240 floats = 40 KB
constexpr int HW_FLOATS = H * MAXA + MAXA + H;  // head weights staged in LDS: actor [64][8] + bias [8] (zero padded), critic [64]
constexpr int LDSX_FLOATS = 2 * CH_FLOATS + WAVES2 * R16 * APITCH + HW_FLOATS;
constexpr int MAX_KX = 256;

struct XArgs {
    FusedArgs f;                  // h_in, bias, zadd*, c_prev, done, gates, c_new, h_new, strides, E, hd
    const float* x; int64_t x_sn, x_row;
    const float* x2; int64_t x2_sn, x2_row;   // optional second piece of x: columns [32 nx1, KX) come from here
    const float* img; int64_t img_sn;
    int nx, nx1, N;               // x chunks (KX / 32), chunks of the first piece, agents
    // message pre-phase (MSG != 0): the LAST 64 columns of x are computed here from the neighbours' previous h
    int msg_kc, m_max;            // chunks of the message input (K_m / 32), neighbour slots
    const int32_t* nbr_idx;       // [N, m_max], -1 padded
    const float* msg_img; int64_t msg_img_sn;     // [K_m][16][4]: image of W_msg (nmarl_lstm_msg_wimage)
    const float* msg_b; int64_t msg_b_sn;         // [N, 64]
    const float* enc; int64_t enc_sn, enc_row;    // MSG 2: the additive h-independent part of the input [N,E,64]
    float* xm_out; int64_t xm_sn, xm_row;         // where the computed 64 columns are kept (may be NULL)
    // HEAD 4 (round 6): the re-step's message term IS the next lock-step's policy-step message term (same neighbours' h, Q3: un-masked)
    // -- carry_out [N][E][64] receives it (before enc is added), carry_in hands the previous launch's over: no neighbour rows, no
    // product in front of the K loop.  mm_next: MSG 2, the re-step's mean rows = the next lock-step's mm_out.  All may be NULL.
    const float* carry_in; int64_t carry_in_sn;
    float* carry_out; int64_t carry_out_sn;
    float* mm_next; int64_t mm_next_sn, mm_next_row;
    float* mm_out; int64_t mm_sn, mm_row;         // MSG 2, may be NULL: where the policy step's mean_j(h_j) rows are kept (the update's
                                                  // message-weight gradient is mean(h)^T D1: no averaging pass over the h sequence there)
    const float* src; int64_t src_sn;             // MSG 3: the senders' message vectors [N,E,64] the pre-phase gathers (instead of h)
    float* xm2_out; int64_t xm2_sn, xm2_row;      // MSG 3: where hm = relu(.) is kept BEFORE enc is added (may be NULL)
    // MSG 3, HEAD 1, nxt_out != NULL: the SENDER layer on the new h, msg' = relu(h' W_mfc + b) -> nxt_out [N,E,64]: what the value
    // re-step and the next lock-step's policy step gather (instead of an fc launch on h' in between)
    const float* nxt_img; int64_t nxt_img_sn;     // nmarl_lstm_msg_wimage of W_mfc [N,64,64]
    const float* nxt_b; int64_t nxt_b_sn;
    float* nxt_out; int64_t nxt_out_sn;
    unsigned* sync;               // HEAD 4: [0] generation, [1] blocks finished, [2] error, [16 + (agent, block, wave)] flags
    // HEAD 4 + MSG 2, ob != NULL: lstm_ic3's observation encoder enc = tanh([x_i | x_nbr] W_ob + b_ob) (agents/utils.py:395-399)
    // runs here as well, from the env's compact observation; its result goes to `enc` (the update needs it) before it is used
    const float* ob; int64_t ob_row;              // [E][N][F] own features per agent, row pitch ob_row floats
    int ob_F, ob_segs;                            // F (multiple of 4), slots = 1 + neighbours: F * slots <= 64 inputs
    const int32_t* ob_nbr;                        // [N, slots]: own index first, then the neighbours ascending, -1 padded
    const float* ob_img; int64_t ob_img_sn;       // image (nmarl_lstm_msg_wimage) of W_ob zero-padded to 64 rows
    const float* ob_b; int64_t ob_b_sn;           // [N, 64]
    int32_t* status;              // HEAD 4, may be NULL: hand-off status words ([0] <- 1 when a wave gives up, sticky)
    unsigned max_spins;           // HEAD 4: polls before a wave gives up
    int fault;                    // HEAD 4 test hook: block 0 never publishes (its neighbours time out)
    // ENC 1: the input encoders of THIS lock-step run here too (see the ENC block of the kernel): x is not read
    const float* e_ob; int64_t e_ob_row;          // the env's compact observation [E][N][5]
    const float* e_fp; int64_t e_fp_sn;           // previous-step policies [N][E][4]
    const float *e_wob, *e_bob, *e_wfp, *e_bfp;   // [N][15][64], [N][64], [N][8][64], [N][64] (the parameter tensors themselves)
    int64_t e_wob_sn, e_bob_sn, e_wfp_sn, e_bfp_sn;
    float* e_out; int64_t e_out_sn, e_out_row;    // where the encoded LSTM input [N][E][128] is kept for the update (may be NULL)
    unsigned* e_bits; int64_t e_bits_sn;          // [N][E][4] words: which of the 128 encoder outputs are > 0 (nmarl_step_enc_t.relu_bits; may be NULL)
    int e_nbr[64];                                // neighbour table [N][2] (-1 padded) BY VALUE: no dependent table load
    int e_ob_rows;                                // rows of w_ob: 15 = 5 x (1 + 2 slots), or 5 (own features only: m_max = 0)
    // ENC 3 / 4 (the encoders on a GENERAL input layout: F own features x (1 + m_max <= 4) slots, A fingerprint entries x m_max; the ATSC
    // grid: 12 x 5 and 5 x 4) take their layout through the SAME words -- the argument block, and with it every other form's code, stays
    // as it was: e_nbr[n] = agent n's four neighbours, one signed byte each (-1: absent; N <= 32); e_ob_rows = rows of w_ob | rows of
    // w_fp << 8 | A << 16; F = ob_F
    // ENC 1 + ev_on: the CACC env step of THIS lock-step behind the action draw (see the ENV block at the end of the kernel)
    int ev_on, ev_auto_reset;
    nmarl_cacc_params_t ev_p;
    float *ev_h, *ev_v, *ev_u; int32_t* ev_t; uint8_t* ev_coll; float* ev_v0;
    float* ev_obs; float* ev_rew; uint8_t* ev_done; float* ev_grew;
    uint64_t ev_seed; int64_t ev_base; int32_t* ev_episode;
    unsigned* ev_cnt;             // [E] hand-off words: bits 0..15 the N agents' draws (2 bits each), bits 16.. the arrivals; zero between launches
    // HEAD 4 + MSG 2 + gv_on (round 6): the synthetic grid's env step as a ROLE of this launch -- blocks >= gv_lstm_blocks (the compute
    // units the 25 x ceil(E / 128) LSTM blocks leave idle) wait for the 25 drawn actions of their replicas and step them while the
    // LSTM blocks run their value re-step (see the GRID ENV block at the kernel's top)
    int gv_on, gv_lstm_blocks, gv_auto_reset;
    nmarl_grid_params_t gv_p;
    float *gv_q, *gv_tr; uint8_t* gv_prev; int32_t* gv_t; float* gv_xi;
    float* gv_obs; float* gv_rew; uint8_t* gv_done; float* gv_grew;
    uint64_t gv_seed; int64_t gv_base; int32_t* gv_episode;
    unsigned long long* gv_words;  // [E][2]: bits 0..38 = 13 agents' draws (3 bits each), bits 59.. = arrivals; zero between launches
};

// raw buffer access for the in-launch hand-off of HEAD 4 (see lstm_bptt.hip for the rules: write-through stores and
// L1-bypassing loads carry the sc1 bit; stores take their offset in a VGPR, never in the scalar-offset field)
typedef unsigned int u32x4v __attribute__((__vector_size__(16)));
typedef __attribute__((address_space(1))) unsigned gu32;
constexpr int SC1 = 16;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* p, const uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, bytes, 0x00020000);
}

// one k-step: 16 MFMAs (all column tiles) with the A value `av` and the B operands in four float4 registers
#define NMARL_MFMA16(av, b0, b1, b2, b3)                                                  \
    {                                                                                     \
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0.x, acc[0], 0, 0, 0);         \
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0.y, acc[1], 0, 0, 0);         \
        acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0.z, acc[2], 0, 0, 0);         \
        acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0.w, acc[3], 0, 0, 0);         \
        acc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1.x, acc[4], 0, 0, 0);         \
        acc[5] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1.y, acc[5], 0, 0, 0);         \
        acc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1.z, acc[6], 0, 0, 0);         \
        acc[7] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1.w, acc[7], 0, 0, 0);         \
        acc[8] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b2.x, acc[8], 0, 0, 0);         \
        acc[9] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b2.y, acc[9], 0, 0, 0);         \
        acc[10] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b2.z, acc[10], 0, 0, 0);       \
        acc[11] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b2.w, acc[11], 0, 0, 0);       \
        acc[12] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b3.x, acc[12], 0, 0, 0);       \
        acc[13] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b3.y, acc[13], 0, 0, 0);       \
        acc[14] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b3.z, acc[14], 0, 0, 0);       \
        acc[15] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b3.w, acc[15], 0, 0, 0);       \
    }
// B operands of k row `krow` of a chunk buffer (lane base already applied): four ds_read_b128
#define NMARL_BLOAD(dst, buf, krow)                                                       \
    {                                                                                     \
        const float4* q_ = reinterpret_cast<const float4*>((buf) + (krow) * 320);         \
        dst##0 = q_[0]; dst##1 = q_[1]; dst##2 = q_[2]; dst##3 = q_[3];                   \
    }
// a whole chunk (8 k-steps) with the B operands of step s + 1 in flight while the MFMAs of step s issue
// (two register sets; sched_barrier keeps the compiler from sinking the reads back behind the MFMAs)
#define NMARL_CHUNK(buf, A0, A1)                                                          \
    {                                                                                     \
        float4 p0, p1, p2, p3, q0, q1, q2, q3;                                            \
        NMARL_BLOAD(p, buf, 0)                                                            \
        NMARL_BLOAD(q, buf, 1) __builtin_amdgcn_sched_barrier(0);                         \
        NMARL_MFMA16(A0.x, p0, p1, p2, p3) __builtin_amdgcn_sched_barrier(0);             \
        NMARL_BLOAD(p, buf, 2) __builtin_amdgcn_sched_barrier(0);                         \
        NMARL_MFMA16(A0.y, q0, q1, q2, q3) __builtin_amdgcn_sched_barrier(0);             \
        NMARL_BLOAD(q, buf, 3) __builtin_amdgcn_sched_barrier(0);                         \
        NMARL_MFMA16(A0.z, p0, p1, p2, p3) __builtin_amdgcn_sched_barrier(0);             \
        NMARL_BLOAD(p, buf, 16) __builtin_amdgcn_sched_barrier(0);                        \
        NMARL_MFMA16(A0.w, q0, q1, q2, q3) __builtin_amdgcn_sched_barrier(0);             \
        NMARL_BLOAD(q, buf, 17) __builtin_amdgcn_sched_barrier(0);                        \
        NMARL_MFMA16(A1.x, p0, p1, p2, p3) __builtin_amdgcn_sched_barrier(0);             \
        NMARL_BLOAD(p, buf, 18) __builtin_amdgcn_sched_barrier(0);                        \
        NMARL_MFMA16(A1.y, q0, q1, q2, q3) __builtin_amdgcn_sched_barrier(0);             \
        NMARL_BLOAD(q, buf, 19) __builtin_amdgcn_sched_barrier(0);                        \
        NMARL_MFMA16(A1.z, p0, p1, p2, p3) __builtin_amdgcn_sched_barrier(0);             \
        NMARL_MFMA16(A1.w, q0, q1, q2, q3)                                                \
    }

// ---- PREC 1 (bf16x3, opt-in): every fp32 operand a = hi + lo with hi = bf16_rne(a), lo = bf16_rne(a - hi); a product is
// hi_a hi_b + hi_a lo_b + lo_a hi_b on v_mfma_f32_16x16x32_bf16 (each bf16 x bf16 product exact in fp32, fp32 accumulation;
// the dropped lo_a lo_b and the two roundings leave ~3 * 2^-18 |a||b| per product).  A chunk's 32 k rows are ONE k-block:
// lane (c, grp) holds A[row c][k = 8 grp + j] and B[k = 8 grp + j][col c], and MFMA k index 8 grp + j is chunk row 4 grp + j
// (j < 4), 16 + 4 grp + j - 4 (j >= 4) -- exactly the rows the lane's fp32 A registers A0 / A1 already hold, so the A fragment
// is those registers split in place; the image (nmarl_lstm_wimage, precision 1) stores B in the same k order.
// Chunk image (same 40 KB as the fp32 one, so the staging ring is unchanged): lane (c, grp) owns X3_PITCH dwords at
// (16 grp + c) X3_PITCH; tile t's hi fragment is dwords 8 t .. 8 t + 3, its lo fragment 8 t + 4 .. 8 t + 7 -- one ds_read_b128
// each; X3_PITCH = 4 x odd keeps the 16 lanes of a group on disjoint banks.
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
constexpr int X3_PITCH = 132;
static_assert(63 * X3_PITCH + 128 <= CH_FLOATS, "bf16x3 chunk image fits the fp32 chunk");

__device__ __forceinline__ void split_bf16x3(const float4 a0, const float4 a1, bf16x8& hi, bf16x8& lo) {
    const float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 h = (__bf16)v[j];          // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
        hi[j] = h;
        lo[j] = (__bf16)(v[j] - (float)h);      // exact difference, rounded once
    }
}

// the three split products of one column tile: small terms first
#define NMARL_MFMA3(ACC, ah, al, bh, bl)                                                  \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, ACC, 0, 0, 0);                  \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, ACC, 0, 0, 0);                  \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, ACC, 0, 0, 0);

// a whole chunk: 16 tiles x 3 MFMAs, the next tile's two ds_read_b128 in flight while one tile multiplies (one tile of look-ahead:
// a second one pushes the policy + value forms, which hold the x-side addend through the K loop, into scratch)
__device__ __forceinline__ void chunk_bf16x3(f32x4 (&acc)[16], const float* buf, const float4 a0, const float4 a1) {
    bf16x8 ah, al;
    split_bf16x3(a0, a1, ah, al);
    const bf16x8* q = reinterpret_cast<const bf16x8*>(buf);      // lane base applied: q[2 t] = hi, q[2 t + 1] = lo of tile t
    bf16x8 p0 = q[0], p1 = q[1], r0 = q[2], r1 = q[3];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 16; t += 2) {
        NMARL_MFMA3(acc[t], ah, al, p0, p1)
        __builtin_amdgcn_sched_barrier(0);
        if (t + 2 < 16) { p0 = q[2 * t + 4]; p1 = q[2 * t + 5]; }
        __builtin_amdgcn_sched_barrier(0);
        NMARL_MFMA3(acc[t + 1], ah, al, r0, r1)
        __builtin_amdgcn_sched_barrier(0);
        if (t + 2 < 16) { r0 = q[2 * t + 6]; r1 = q[2 * t + 7]; }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// MSG: the message term of a coupled net computed IN the step kernel (no gather / GEMM / bias-activation launches):
//   1  lstm_comm (agents/utils.py:182-199):  hm = relu([h_j : j in nbr(i)] @ W_msg + b_msg)          -> x[:, KX-64:]
//   2  lstm_ic3  (agents/utils.py:395-400):  s  = mean_j(h_j) @ W_msg + b_msg + enc                   -> x (KX = 64)
//   3  lstm_dial (agents/utils.py:515-599):  hm = relu([msg_j : j in nbr(i)] @ W_msg + b_msg), s = hm + enc -> x (KX = 64);
//      msg_j = relu(h_j W_mfc + b) is the SENDER's layer, one fc launch of the caller (xa.src), gathered here like MSG 1's h
// from the neighbours' PREVIOUS, un-masked h (quirk Q3): h_in of the other agents, complete before this launch.
// A pre-phase on the matrix cores ([16 rows x K_m] @ [K_m x 64], A operands gathered from global memory, W_msg from an
// LDS image staged behind the chunk buffers); its result goes through the wave's LDS tile into A layout, where the
// main K loop picks it up as its last two x chunks, and (policy step) to global memory for the update's backward.

// ENC 1 (uncoupled nets on CACC, IA2C-FP: KX = 128 = [relu(x~ W_ob + b) | relu(p~ W_fp + b)], policies.py:176-181): the two
// input encoders run HERE, as a register-only pre-phase, instead of in a launch of their own in front of every lock-step
// (fc_fwd_multi / the tail of cacc_step_encode_kernel: ~6 us of latency and a 16.8-MB write + re-read per lock-step at
// 8 x 4096 rows).  The product is taken TRANSPOSED, S^T = W^T x~^T, on v_mfma_f32_16x16x4_f32: the matrix-A operand is a
// 16-column slice of W (lane (i, k) reads W[4 s + k][16 mt + i] straight from the parameter tensor: no image, no LDS), the
// matrix-B operand is the input x~[row][4 s + k] (lane (row, k): one float per k-step, gathered from the env's compact
// observation [own | nbr 0 | nbr 1] x 5 features, one zero pad, then the two neighbours' 4-wide fingerprints: 24 inputs = 6
// k-steps; W is block diagonal, so 4 x 4 + 4 x 2 = 24 MFMAs), and the C/D layout of the result hands lane (row, grp) the
// columns 16 mt + 4 grp + {0..3} of ITS row -- exactly the A-operand layout of the main K loop (k = 32 ch + 16 jj + 4 grp
// + {0..3}, mt = 2 ch + jj).  No cross-lane movement at all: the 32 values per lane are parked in a lane-private LDS slot
// (the register file is full: 254 VGPRs) over the not-yet-used h' tile, and written once to the saved activations.
// Two chunk buffers instead of three (no de-phased wave groups: measured +-0 in round 2) make the room.
// CARRY (HEAD 4, round 6): 0 none; 1 the re-step hands its message term on (carry_out / mm_next); 2 it also STARTS from the one the
// previous launch handed on (carry_in): no neighbour rows, no product in front of the K loop.  A template parameter, not a launch
// argument: at 256 registers a run-time choice cost every form of the kernel ~4 us (profiles/r06_ab_msg_carry.txt).
// PREC (opt-in): 0 exact fp32 (v_mfma_f32_16x16x4_f32), 1 bf16x3 for the main K loop and the value re-step's h' @ Wh (see
// chunk_bf16x3; img is then nmarl_lstm_wimage's precision-1 image).  The encoder pre-phase, epilogues and heads stay fp32.
template <int HEAD, int MSG, int ENC = 0, int CARRY = 0, int PREC = 0>
__global__ __launch_bounds__(512, 1) void lstm_step_x_kernel(const XArgs xa) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const FusedArgs& a = xa.f;
    NMARL_STAMP(0)
    constexpr bool GENV = HEAD == 4 && MSG == 2;             // the grid's env step can be a role of this launch
    const unsigned n_lstm = (GENV && xa.gv_on) ? (unsigned)xa.gv_lstm_blocks : gridDim.x;
    if (GENV && xa.gv_on && blockIdx.x >= n_lstm) {
        // ---- GRID ENV role (envs/atsc_env.py:181-207 on the synthetic dynamics of oracle/grid_ref.py): this block is not an LSTM
        // block.  Groups of 16 replicas (one per half wave): wait until all 25 agents' waves have added their draws into the
        // replica's two hand-off words (the LSTM blocks do so right behind their actor heads), then grid_step_groups -- the env
        // kernel's own device function -- writes state, reward, done and the compact observation of lock-step t + 1 while the LSTM
        // blocks are still in their value re-steps.  Bounded waits; a time-out raises the hand-off status word (fail closed).
        nmarl_grid::Lds* el = reinterpret_cast<nmarl_grid::Lds*>(lds);
        float* bq = reinterpret_cast<float*>(el + 16);
        float* bt = bq + 16 * nmarl_grid::NQ;
        nmarl_grid::grid_step_groups<0, true, false, 16, true>(
            xa.gv_p, a.E, (int64_t)(blockIdx.x - n_lstm), (int64_t)(gridDim.x - n_lstm), nullptr, xa.gv_words, xa.status, xa.max_spins, xa.gv_q,
            xa.gv_tr, xa.gv_prev, xa.gv_t, xa.gv_xi, xa.gv_obs, xa.gv_rew, xa.gv_done, xa.gv_grew, xa.gv_auto_reset, xa.gv_seed, xa.gv_base,
            xa.gv_episode, el, bq, bt, bt);
        return;
    }
    int n, blk_u;
    nmarl_xcd_work(blockIdx.x, n_lstm, a.blocks_per_agent, n, blk_u);             // an agent's blocks share an XCD (its L2 holds the image)
    // ENC: touch every scalar-cache line of the launch arguments (1.1 KB: 18 lines) with one back-to-back burst of scalar loads; the
    // values are consumed (or-ed into nothing) only at the end of the prologue, so the lines arrive while the vector loads issue --
    // the compiler's lazy argument loads then hit the scalar cache instead of each paying a first-touch miss behind its own wait
    unsigned ka_touch = 0;
    if (ENC) {
        const __attribute__((address_space(4))) unsigned* ka =
            (const __attribute__((address_space(4))) unsigned*)__builtin_amdgcn_kernarg_segment_ptr();
#pragma unroll
        for (unsigned o = 0; o < sizeof(XArgs); o += 64) ka_touch |= ka[o / 4];
    }
    // ENC: every launch argument the encoder pre-phase needs, fetched NOW in one batch of scalar loads.  Left to the compiler they
    // are loaded where first used, one at a time, each behind its own wait: the argument block spans many scalar-cache lines, and
    // three such first-touch misses in a row in front of the pre-phase's loads cost ~5 k cycles (tools/step_timeline.py enc)
    const float* const e_ob = xa.e_ob; const float* const e_fp = xa.e_fp;
    const float* const e_wob = xa.e_wob; const float* const e_bob = xa.e_bob;
    const float* const e_wfp = xa.e_wfp; const float* const e_bfp = xa.e_bfp;
    float* const e_out = xa.e_out;
    unsigned* const e_bits = xa.e_bits;
    const int64_t e_bits_sn = xa.e_bits_sn;
    const int64_t e_ob_row = xa.e_ob_row, e_fp_sn = xa.e_fp_sn, e_wob_sn = xa.e_wob_sn, e_bob_sn = xa.e_bob_sn, e_wfp_sn = xa.e_wfp_sn,
                  e_bfp_sn = xa.e_bfp_sn, e_out_sn = xa.e_out_sn, e_out_row = xa.e_out_row;
    int e_nb0 = -1, e_nb1 = -1;
    int e_nb2 = -1, e_nb3 = -1;                  // ENC 3 / 4: up to four neighbour slots
    if (ENC >= 3) {
        const int ns_ = __builtin_amdgcn_readfirstlane(n);
        const int nb4_ = xa.e_nbr[ns_];                              // four signed bytes
        e_nb0 = (nb4_ << 24) >> 24; e_nb1 = (nb4_ << 16) >> 24; e_nb2 = (nb4_ << 8) >> 24; e_nb3 = nb4_ >> 24;
        asm volatile("" :: "s"(e_ob), "s"(e_fp), "s"(e_wob), "s"(e_bob), "s"(e_wfp), "s"(e_bfp), "s"(e_out), "s"(e_ob_row), "s"(e_fp_sn),
                     "s"(e_wob_sn), "s"(e_bob_sn), "s"(e_wfp_sn), "s"(e_bfp_sn), "s"(e_out_sn), "s"(e_out_row), "s"(e_nb0), "s"(e_nb1), "s"(e_nb2),
                     "s"(e_nb3), "s"(e_bits), "s"(e_bits_sn));
    } else if (ENC) {
        const int ns_ = __builtin_amdgcn_readfirstlane(n);
        e_nb0 = xa.e_nbr[2 * ns_]; e_nb1 = xa.e_nbr[2 * ns_ + 1];
        asm volatile("" :: "s"(e_ob), "s"(e_fp), "s"(e_wob), "s"(e_bob), "s"(e_wfp), "s"(e_bfp), "s"(e_out), "s"(e_ob_row), "s"(e_fp_sn),
                     "s"(e_wob_sn), "s"(e_bob_sn), "s"(e_wfp_sn), "s"(e_bfp_sn), "s"(e_out_sn), "s"(e_out_row), "s"(e_nb0), "s"(e_nb1), "s"(e_bits),
                     "s"(e_bits_sn));
    }
    const int64_t row_blk = (int64_t)blk_u * ROWS_B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = row_blk + wave * R16;
    const int c = lane & 15, grp = lane >> 4;
    // (a static s_setprio 1 for the younger wave group 4..7 of the coupled kernels -- MI355X_MICROARCH.md's lever for 8-wave blocks --
    // was tried in round 6: +0.3 % on the grid's lock-step, same box: not kept)
    static_assert(HEAD != 4 || MSG != 0, "HEAD 4 is the coupled nets' policy + value step");
    static_assert(PREC == 0 || MSG == 0, "bf16x3: the uncoupled nets' step forms only");
    constexpr bool PV = HEAD == 3 || HEAD == 4;          // policy step + value re-step in this launch
    // HEAD 4: this launch's flag value = generation + 1.  The load is ISSUED here and consumed after the K loop: a
    // readfirstlane right away would park the wave for a memory round trip before it has requested anything else
    unsigned epoch_raw = 0;
    if (HEAD == 4) epoch_raw = __hip_atomic_load((gu32*)xa.sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the neighbour tables of this agent (uniform): every entry requested NOW, back to back -- looked up where they are used,
    // each one costs a dependent (scalar) memory round trip in front of the loads it addresses
    int nbj[8];
    if (MSG != 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) nbj[k] = xa.nbr_idx[n * xa.m_max + (k < xa.m_max ? k : 0)];
    }
    // the message layer's bias and the observation encoder's (lane column c = units 4 c .. 4 c + 3): requested here too -- loaded
    // where they are added, each exposes a memory round trip inside a pre-phase
    constexpr bool OBENC = HEAD == 4 && MSG == 2;                    // the in-kernel observation encoder exists (runs if xa.ob)
    const bool ob_here = OBENC && xa.ob != nullptr;
    float4 bv4 = float4{0.f, 0.f, 0.f, 0.f}, bo4 = float4{0.f, 0.f, 0.f, 0.f};
    if (MSG != 0) {
        const float* mbias_ = xa.msg_b + (int64_t)n * xa.msg_b_sn;
        bv4 = *reinterpret_cast<const float4*>(mbias_ + 4 * (lane & 15));
        if (OBENC) bo4 = *reinterpret_cast<const float4*>((ob_here ? xa.ob_b + (int64_t)n * xa.ob_b_sn : mbias_) + 4 * (lane & 15));
    }
    NMARL_STAMP(40)
    // De-phased wave groups (no message pre-phase only: LDS): waves 4-7 run ONE chunk behind waves 0-3 through a ring
    // of three chunk buffers, so that on every SIMD one wave's VALU epilogue / head overlaps the other's MFMAs instead
    // of both epilogues running side by side with an idle matrix pipe.
    constexpr bool DEPH = MSG == 0 && ENC == 0;
    constexpr int NBUF = DEPH ? 3 : 2;
    static_assert(ENC == 0 || (MSG == 0 && HEAD == 3) || (ENC == 1 && MSG == 1 && HEAD == 4), "ENC: the policy + value launch of IA2C(-FP) / ConseNet / NeurComm");
    static_assert(ENC >= 0 && ENC <= 4 && (ENC < 3 || PREC == 0), "ENC 3 / 4 (general input layout): fp32 only");
    // ENC 1: two encoders [relu(x~ W_ob + b) | relu(p~ W_fp + b)] (128 outputs: IA2C-FP, NeurComm); ENC 2 (round 6): the observation
    // encoder alone (64 outputs: IA2C policies.py:145; ConseNet policies.py:381-390 with its own features only = no neighbour slots)
    // ENC 3 / 4: the same two forms on a GENERAL input layout (EGEN, see the pre-phase behind the prologue's barrier)
    constexpr bool EFP = ENC == 1 || ENC == 3;
    constexpr bool EGEN = ENC >= 3;
    constexpr int EMT = EFP ? 8 : 4;                      // 16-column m-tiles of the encoders' output
    // Where the encoders' 128 outputs wait for the K loop: ENC_LDS (uncoupled nets) in lane-private LDS slots; ENC_GLB (NeurComm: the
    // message image and the parked cell state leave no 64 KB of LDS) in the S slot of the saved activations itself -- every lane
    // stores its 8 x 16 bytes there (the update needs them anyway) and the K loop's ordinary A loads read them back: the SAME lane
    // reads exactly the addresses it wrote (C/D layout of the transposed product == A layout of the K loop), program order.
    constexpr bool ENC_LDS = ENC != 0 && MSG == 0, ENC_GLB = ENC != 0 && MSG != 0;
    // ENC: [chunks][head weights][union(h' tiles, lane-private x slots: 8 float4 x 512 threads)] -- the tiles are first written in
    // the cell epilogue, behind the last tick's barrier, when every wave has consumed its x chunks
    float* hw_lds = ENC_LDS ? lds + NBUF * CH_FLOATS : lds + NBUF * CH_FLOATS + WAVES2 * R16 * APITCH;   // head weights: [64][A] actor, then [64] critic
    float* a_tile = (ENC_LDS ? hw_lds + HW_FLOATS : lds + NBUF * CH_FLOATS) + wave * R16 * APITCH;
    float4* xslot = reinterpret_cast<float4*>(hw_lds + HW_FLOATS) + threadIdx.x;            // ENC: + 512 q, q = 0..7
    const int nx = xa.nx, nch = xa.nx + 2;
    const float4* img = reinterpret_cast<const float4*>(xa.img + (int64_t)n * xa.img_sn);

    // ---- W chunk staging: 2560 float4 per chunk = 5 per thread, image order == LDS order
    // (five NAMED registers: as an array living across the runtime chunk loop the compiler demotes it to scratch)
    float4 sg0, sg1, sg2, sg3, sg4;
#define NMARL_STAGE_LOAD(ch)                                                              \
    {                                                                                     \
        const float4* g_ = img + (int64_t)(ch) * (CH_FLOATS / 4) + threadIdx.x;           \
        sg0 = g_[0]; sg1 = g_[512]; sg2 = g_[1024]; sg3 = g_[1536]; sg4 = g_[2048];       \
    }
#define NMARL_STAGE_STORE(b)                                                              \
    {                                                                                     \
        float4* d_ = reinterpret_cast<float4*>(lds + (b) * CH_FLOATS) + threadIdx.x;      \
        d_[0] = sg0; d_[512] = sg1; d_[1024] = sg2; d_[1536] = sg3; d_[2048] = sg4;       \
    }
    NMARL_STAGE_LOAD(0)
    float4 tg0, tg1, tg2, tg3, tg4;              // chunk 1, in flight together with chunk 0 (prologue only)
    {
        const float4* g_ = img + (CH_FLOATS / 4) + threadIdx.x;
        tg0 = g_[0]; tg1 = g_[512]; tg2 = g_[1024]; tg3 = g_[1536]; tg4 = g_[2048];
    }

    // ---- A operands: row (lane & 15) of this wave's strip, k = 32 ch + 16 j + 4 grp + {0..3}
    const int64_t arow = row0 + c < a.E ? row0 + c : a.E - 1;
    const float keepA = 1.0f - a.done[arow];
    const float* xrow = xa.x ? xa.x + (int64_t)n * xa.x_sn + arow * xa.x_row + 4 * grp : nullptr;
    const float* x2row = xa.x2 ? xa.x2 + (int64_t)n * xa.x2_sn + arow * xa.x2_row + 4 * grp : nullptr;
    const int nx1 = xa.nx1;
    const float* hrow = a.h_in + (int64_t)n * a.h_sn + arow * H + 4 * grp;
    float4 a0, a1, n0, n1;
#define NMARL_A_LOAD(ch, d0, d1)     /* raw load; the (1 - done) mask of the h chunks is applied at first use */ \
    if (ENC_LDS) {      /* x chunks: the lane's own slots; h chunks: global.  BOTH requested unconditionally (clamped), then selected */ \
        const int hc_ = (ch) - nx < 0 ? 0 : (ch) - nx;                                    \
        const int xc_ = (ch) < nx ? (ch) : nx - 1;                                        \
        const float4 h0_ = *reinterpret_cast<const float4*>(hrow + hc_ * CH_K);           \
        const float4 h1_ = *reinterpret_cast<const float4*>(hrow + hc_ * CH_K + 16);      \
        const float4 x0_ = xslot[512 * (2 * xc_)], x1_ = xslot[512 * (2 * xc_ + 1)];      \
        const bool isx_ = (ch) < nx;                                                      \
        d0.x = isx_ ? x0_.x : h0_.x; d0.y = isx_ ? x0_.y : h0_.y; d0.z = isx_ ? x0_.z : h0_.z; d0.w = isx_ ? x0_.w : h0_.w; \
        d1.x = isx_ ? x1_.x : h1_.x; d1.y = isx_ ? x1_.y : h1_.y; d1.z = isx_ ? x1_.z : h1_.z; d1.w = isx_ ? x1_.w : h1_.w; \
    } else if (MSG != 0 && (ch) >= nx - 2 && (ch) < nx) {       /* the message columns: from the wave's LDS tile */ \
        const float* t_ = a_tile + c * APITCH + ((ch) - (nx - 2)) * CH_K + 4 * grp;       \
        d0.x = t_[0]; d0.y = t_[1]; d0.z = t_[2]; d0.w = t_[3];                           \
        d1.x = t_[16]; d1.y = t_[17]; d1.z = t_[18]; d1.w = t_[19];                       \
    } else if ((ch) < nx) {                                                               \
        const float* p_ = (ch) < nx1 ? xrow + (ch) * CH_K : x2row + ((ch) - nx1) * CH_K;  \
        d0 = *reinterpret_cast<const float4*>(p_);                                        \
        d1 = *reinterpret_cast<const float4*>(p_ + 16);                                   \
    } else {                                                                              \
        d0 = *reinterpret_cast<const float4*>(hrow + ((ch) - nx) * CH_K);                 \
        d1 = *reinterpret_cast<const float4*>(hrow + ((ch) - nx) * CH_K + 16);            \
    }
#define NMARL_A_MASK(ch, d0, d1)                                                          \
    {                                                                                     \
        const float kf_ = (ch) < nx ? 1.0f : keepA;                                       \
        d0.x *= kf_; d0.y *= kf_; d0.z *= kf_; d0.w *= kf_;                               \
        d1.x *= kf_; d1.y *= kf_; d1.z *= kf_; d1.w *= kf_;                               \
    }
    // one chunk of the main product from the chunk buffer at CB (the lane's base applied here): fp32 or bf16x3 (PREC)
#define NMARL_KCHUNK(CB, A0, A1)                                                          \
    if constexpr (PREC != 0) {                                                            \
        chunk_bf16x3(acc, (CB) + (16 * grp + c) * X3_PITCH, A0, A1);                      \
    } else {                                                                              \
        const float* buf = (CB) + (4 * grp * 16 + c) * 20;                                \
        NMARL_CHUNK(buf, A0, A1)                                                          \
    }
    if (MSG == 0 && ENC == 0) { NMARL_A_LOAD(0, a0, a1) }
    // ---- ENC: the input encoders' operands (see the kernel's header), REQUESTED here -- behind the two weight chunks, in front of
    // everything else the prologue asks for -- and consumed just before the prologue's barrier
    float ein[ENC == 3 ? 24 : ENC == 4 ? 16 : ENC == 1 ? 6 : (ENC ? 4 : 1)];
    float ewt[ENC == 3 ? 12 : ENC == 4 ? 8 : ENC == 1 ? 3 : (ENC ? 2 : 1)];
    f32x4 eacc[EFP ? 8 : (ENC ? 4 : 1)];
    if constexpr (EGEN) {
        // ---- ENC 3 / 4: F own features x (1 + m_max) observation slots (k-steps 0 .. obk - 1: F is a multiple of 4, so a k-step's four
        // inputs are features f0 .. f0 + 3 of ONE slot, whose agent is uniform; lane group grp = the feature) and A fingerprint entries
        // x m_max neighbours (k-steps 0 .. fpk - 1 of the second product: input 4 s + grp = entry (4 s + grp) % A of slot (4 s + grp) / A,
        // per lane).  Slot k + 1 is neighbour k of the by-value table; an absent slot contributes 0 (its address falls back to the
        // agent's own first entries: always inside the tensors).  Inputs in their natural order = the weight rows' order.
        __builtin_amdgcn_sched_barrier(0);                                // (the chunk loads above stay first)
        const int ns = __builtin_amdgcn_readfirstlane(n);
        const int F = xa.ob_F, A = (xa.e_ob_rows >> 16) & 255, fp_rows = (xa.e_ob_rows >> 8) & 255;
        const int obk = (xa.e_ob_rows & 255) >> 2, fpk = (fp_rows + 3) >> 2;  // k-steps of the two products: <= 16, <= 8
        {
            const float* obr = e_ob + arow * e_ob_row + grp;
            int slot = 0, f0 = 0;
#pragma unroll
            for (int s_ = 0; s_ < 16; ++s_) {
                int ag = ns;
                ag = slot == 1 ? e_nb0 : ag; ag = slot == 2 ? e_nb1 : ag; ag = slot == 3 ? e_nb2 : ag; ag = slot == 4 ? e_nb3 : ag;
                const bool ok = s_ < obk && ag >= 0;
                const float v = obr[ok ? ag * F + f0 : ns * F];
                ein[s_] = ok ? v : 0.0f;
                f0 += 4;
                if (f0 >= F) { f0 = 0; ++slot; }
            }
            if constexpr (EFP) {
#pragma unroll
                for (int s_ = 0; s_ < 8; ++s_) {
                    const int kk = 4 * s_ + grp;
                    const int sl = (kk >= A ? 1 : 0) + (kk >= 2 * A ? 1 : 0) + (kk >= 3 * A ? 1 : 0);
                    int ag = e_nb0;
                    ag = sl == 1 ? e_nb1 : ag; ag = sl == 2 ? e_nb2 : ag; ag = sl == 3 ? e_nb3 : ag;
                    const bool ok = s_ < fpk && kk < fp_rows && ag >= 0;
                    const float v = e_fp[(int64_t)(ok ? ag : ns) * e_fp_sn + arow * A + (ok ? kk - sl * A : 0)];
                    ein[16 + s_] = ok ? v : 0.0f;
                }
            }
        }
        // W -> LDS image [k-step s][lane][m-tile] (the order the lanes read it back in: one ds_read_b128 per k-step), the observation
        // encoder's 16 k-steps first, the fingerprint encoder's 8 behind them.  Rows past the tensors' last (the fingerprint product's
        // last k-step when A m_max is no multiple of 4) are clamped to it: their input is 0.  A wave fetches one whole 256-byte row.
#pragma unroll
        for (int q = 0; q < (EFP ? 12 : 8); ++q) {
            const int e = (q < 8 ? q : q - 8) * 512 + (int)threadIdx.x;
            const int s_ = e >> 8, l_ = (e >> 2) & 63, mt_ = e & 3, g_ = l_ >> 4, i_ = l_ & 15;
            const bool live = s_ < (q < 8 ? obk : fpk);
            int row = 4 * s_ + g_;
            row = q < 8 ? row : (row < fp_rows ? row : fp_rows - 1);
            const float* src = q < 8 ? e_wob + (int64_t)n * e_wob_sn : e_wfp + (int64_t)n * e_wfp_sn;
            ewt[q] = src[(live ? row : 0) * H + 16 * mt_ + i_];
        }
        float4 eb4 = float4{0.f, 0.f, 0.f, 0.f};
        if (threadIdx.x < (EFP ? 32 : 16))
            eb4 = *reinterpret_cast<const float4*>((threadIdx.x < 16 ? e_bob + (int64_t)n * e_bob_sn : e_bfp + (int64_t)n * e_bfp_sn - H) + 4 * threadIdx.x);
        eacc[0] = f32x4{eb4.x, eb4.y, eb4.z, eb4.w};                     // (parked in eacc[0] until it is stored to LDS)
        __builtin_amdgcn_sched_barrier(0);
    } else if (ENC) {
        __builtin_amdgcn_sched_barrier(0);                                // (the chunk loads above stay first)
        const int i16 = lane & 15;
        const int ns = __builtin_amdgcn_readfirstlane(n);                // uniform; the table entries came as scalar loads from the
        const int nb0 = e_nb0, nb1 = e_nb1;                              // launch arguments (no dependent global load)
        // The 24 inputs are ORDERED for cheap addressing (any order serves: the weight rows are fetched to match): k-step s = 0, 1, 2
        // = features 0..3 of slot s (own, neighbour 0, neighbour 1: the slot's agent is uniform, lane group grp = the feature),
        // k-step 3 = feature 4 of slot grp (grp 3: the zero pad), k-steps 4, 5 = the two neighbours' policies (grp = the action).
        // Weight row of (s < 3, grp) = 5 s + grp, of (3, grp) = 5 grp + 4; one per-lane base pointer + compile-time offsets each.
        {
            const float* obr = e_ob + arow * e_ob_row + grp;       // [N][5] of row `arow`, feature grp
            const int ag1 = nb0 >= 0 ? nb0 : ns, ag2 = nb1 >= 0 ? nb1 : ns;
            const float v0 = obr[ns * 5], v1 = obr[ag1 * 5], v2 = obr[ag2 * 5];
            const int ag3 = grp == 0 ? ns : (grp == 1 ? ag1 : ag2);      // (grp 3: a valid dummy)
            const float v3 = e_ob[arow * e_ob_row + ag3 * 5 + 4];
            const bool ok3 = grp == 0 || (grp == 1 && nb0 >= 0) || (grp == 2 && nb1 >= 0);
            ein[0] = v0; ein[1] = nb0 >= 0 ? v1 : 0.0f; ein[2] = nb1 >= 0 ? v2 : 0.0f; ein[3] = ok3 ? v3 : 0.0f;
            if (EFP) {
                const float* fpr = e_fp + arow * 4 + grp;
                const float p0 = fpr[(int64_t)ag1 * e_fp_sn], p1 = fpr[(int64_t)ag2 * e_fp_sn];
                ein[4] = nb0 >= 0 ? p0 : 0.0f; ein[5] = nb1 >= 0 ? p1 : 0.0f;
            }
        }
        // W and the two biases go through LDS: fetched ONCE per block (3 + 1/16 loads per thread, coalesced rows) instead of 24 + 8
        // scattered loads per lane -- the pre-phase was bound by the number of vector-memory instructions the CU's eight waves
        // issue (tools/step_timeline.py enc).  Image order = the order the lanes read it back in: [k-step s][lane][m-tile] floats.
        const int ob_rows = xa.e_ob_rows;                                // 15, or 5 when the net sees its own features only (all slots
#pragma unroll                                                           // absent: their inputs are 0, their weight rows clamped to valid ones)
        for (int q = 0; q < (EFP ? 3 : 2); ++q) {
            const int e = q * 512 + (int)threadIdx.x;                    // 0 .. 1535 = 6 k-steps x 64 lanes x 4 m-tiles (ENC 2: 4 k-steps)
            const int s_ = e >> 8, l_ = (e >> 2) & 63, mt_ = e & 3, g_ = l_ >> 4, i_ = l_ & 15;
            int row = s_ < 3 ? 5 * s_ + g_ : (s_ == 3 ? 5 * (g_ < 3 ? g_ : 2) + 4 : 4 * (s_ - 4) + g_);   // (pad lane: a valid row, its input is 0)
            row = s_ < 4 && row >= ob_rows ? ob_rows - 1 : row;
            const float* src = (s_ < 4 || !EFP) ? e_wob + (int64_t)n * e_wob_sn : e_wfp + (int64_t)n * e_wfp_sn;
            ewt[q] = src[row * H + 16 * mt_ + i_];
        }
        float4 eb4 = float4{0.f, 0.f, 0.f, 0.f};
        if (threadIdx.x < (EFP ? 32 : 16))
            eb4 = *reinterpret_cast<const float4*>((threadIdx.x < 16 ? e_bob + (int64_t)n * e_bob_sn : e_bfp + (int64_t)n * e_bfp_sn - H) + 4 * threadIdx.x);
        eacc[0] = f32x4{eb4.x, eb4.y, eb4.z, eb4.w};                     // (parked in eacc[0] until it is stored to LDS)
        __builtin_amdgcn_sched_barrier(0);
        NMARL_STAMP(36)
    }
    int64_t rofs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + 4 * grp + r;
        rofs[r] = row < a.E ? row : a.E - 1;
    }
    // (chunk 2 is requested at the END of the prologue: vector loads return in order, so asked for here its 40 KB would sit in front
    // of every operand the pre-phases wait for -- it is first needed behind tick 0's barrier, a whole pre-phase + tick away)
    float* m_lds = hw_lds + HW_FLOATS;                               // W_msg image: msg_kc * 32 * 64 floats
    // the heads' h-weights -> LDS (read 16 x (A + 1) times per lane in the head epilogues): REQUESTED here (unconditional,
    // clamped addresses), stored to LDS at the end of the prologue -- stored right away they cost their own round trip
    float hw0 = 0.0f, hw1 = 0.0f, hw2 = 0.0f;
    if (HEAD != 0) {
        const nmarl_head_t& hd = a.hd;
        const float* w1 = hd.w + (int64_t)n * hd.w_sn;
        if (HEAD == 2) {                                     // critic only: [64]
            hw2 = w1[threadIdx.x & (H - 1)];
        } else {                                             // actor [64][A] -> [64][MAXA] zero padded, bias [A] -> [MAXA]
            const int A = hd.A;
            const int k = threadIdx.x >> 3, o = threadIdx.x & 7;               // 512 threads = 64 x 8
            hw0 = w1[k * A + (o < A ? o : 0)];
            hw1 = (hd.b + (int64_t)n * hd.b_sn)[(threadIdx.x & 7) < A ? (threadIdx.x & 7) : 0];
            if (PV) hw2 = (hd.w2 + (int64_t)n * hd.w2_sn)[threadIdx.x & (H - 1)];
        }
    }
    NMARL_STAMP(44)
    float* o_lds = m_lds + xa.msg_kc * (CH_K * 64);                  // W_ob image: 64 x 64 floats
    // the W_msg / W_ob images: all pieces requested at once (a run-time loop would wait for every piece before asking for the next)
    constexpr int MIQ = MSG == 2 ? 2 : 4;                            // pieces per thread: K_m <= 128 (MSG 1 / 3), = 64 (MSG 2)
    float4 mi[MSG != 0 ? MIQ : 1], oi[OBENC ? 2 : 1];
    if (MSG != 0) {
        const float4* g = reinterpret_cast<const float4*>(xa.msg_img + (int64_t)n * xa.msg_img_sn);
        const int lim = xa.msg_kc * (CH_K * 64 / 4);                 // <= 2048 float4 = 4 per thread
#pragma unroll
        for (int q = 0; q < MIQ; ++q) { const int i = threadIdx.x + 512 * q; mi[q] = g[i < lim ? i : 0]; }
    }
    if (OBENC) {
        const float4* g = ob_here ? reinterpret_cast<const float4*>(xa.ob_img + (int64_t)n * xa.ob_img_sn) : img;
#pragma unroll
        for (int q = 0; q < 2; ++q) oi[q] = g[threadIdx.x + 512 * q];
    }
    // the sender layer of the new h (lstm_dial's policy step): its image and bias requested here, stored over the W_msg image
    // once the K loop is through (every wave has left the pre-phase by then)
    constexpr bool NXT = HEAD == 1 && MSG == 3;
    const bool nxt_here = NXT && xa.nxt_out != nullptr;
    // (named registers: an array living across the runtime chunk loop is demoted to scratch, like the staging registers above)
    float4 nfa = float4{0.f, 0.f, 0.f, 0.f}, nfb = nfa, nb4 = nfa;
    if (NXT) {
        const float4* g = nxt_here ? reinterpret_cast<const float4*>(xa.nxt_img + (int64_t)n * xa.nxt_img_sn) : img;
        nfa = g[threadIdx.x]; nfb = g[threadIdx.x + 512];
        nb4 = *reinterpret_cast<const float4*>((nxt_here ? xa.nxt_b + (int64_t)n * xa.nxt_b_sn : xa.msg_b + (int64_t)n * xa.msg_b_sn) + 4 * (lane & 15));
    }
    // msg_load: request the neighbour rows of one round (MSG 1: both slots, all four half-chunks; MSG 2: neighbours k0 .. k0 + 3,
    // both chunks) -- every row BEFORE the first product, absent slots read the own row with weight 0 (no load inside a branch).
    // U: MSG 1 [kc][half], MSG 2 [q][kc][half].
    auto msg_load = [&](auto second_c, auto k0_c, float4 (&U)[16], float (&W)[4]) {
        constexpr bool SECOND = decltype(second_c)::value;
        constexpr int k0 = decltype(k0_c)::value;
        const float* hsrc = MSG == 3 ? xa.src : SECOND ? a.h_new : a.h_in;
        const int64_t hsn = MSG == 3 ? xa.src_sn : SECOND ? a.h_new_sn : a.h_sn;
        const float* hbase = hsrc + arow * H + 4 * grp;              // + j * hsn: row `arow` of agent j
        const uint32_t hoff = (uint32_t)((arow * H + 4 * grp) * 4), hbytes = (uint32_t)(a.E * (H * 4));
        auto load2 = [&](const int jj, const int col, float4& u0, float4& u1) {
            if (SECOND) {
                const __amdgpu_buffer_rsrc_t r_ = make_rsrc(hsrc + (int64_t)jj * hsn, hbytes);
                u0 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r_, hoff + col * 4, 0, SC1));
                u1 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r_, hoff + col * 4 + 64, 0, SC1));
            } else {
                const float* p_ = hbase + (int64_t)jj * hsn + col;
                u0 = *reinterpret_cast<const float4*>(p_);
                u1 = *reinterpret_cast<const float4*>(p_ + 16);
            }
        };
#pragma unroll
        for (int q = 0; q < (MSG == 2 ? 4 : 2); ++q) {
            const int k = k0 + q;
            const int j = nbj[k];
            const bool ok = k < xa.m_max && j >= 0;
            W[q] = ok ? 1.0f : 0.0f;
            load2(ok ? j : n, 0, U[4 * q + 0], U[4 * q + 1]);
            load2(ok ? j : n, CH_K, U[4 * q + 2], U[4 * q + 3]);
        }
    };
    // the first pre-phase's neighbour rows (and the encoder's observation pieces): requested here, consumed after the barrier
    float4 PU[16];
    float PW[4];
    using K0 = std::integral_constant<int, 0>;
    using K2 = std::integral_constant<int, 2>;
    using K4 = std::integral_constant<int, 4>;
    // lstm_comm's launch-per-step forms take a message input of up to 256 floats (four neighbour slots): see msg_phase
    constexpr bool MSG_WIDE = HEAD != 4 && MSG == 1;
    static_assert(CARRY == 0 || (HEAD == 4 && (MSG == 1 || MSG == 2)), "the message carry exists between one-launch lock-steps");
    constexpr bool carried = CARRY == 2;                             // the previous launch's re-step computed this message term
    if (MSG != 0) {
        if (carried) {                      // the lane's four rows of it (C layout), nothing else
            const float* ci = xa.carry_in + (int64_t)n * xa.carry_in_sn + 4 * c;
#pragma unroll
            for (int r = 0; r < 4; ++r) PU[r] = *reinterpret_cast<const float4*>(ci + rofs[r] * H);
            PW[0] = PW[1] = PW[2] = PW[3] = 0.0f;
        } else {
            msg_load(std::false_type{}, K0{}, PU, PW);
        }
    }
    float4 ea[OBENC ? 4 : 1];
    float eaw[OBENC ? 4 : 1];
    if (OBENC) {
        // unconditional loads (a valid dummy row when the encoder does not run): input k = F slot + f, four features of one slot
        const float* obr = ob_here ? xa.ob + arow * xa.ob_row : hrow;
        const int F = ob_here ? xa.ob_F : 64, segs = ob_here ? xa.ob_segs : 0;
        // slot owners: own index, then the neighbour table (ob_nbr [N, segs] = [own | neighbours] by contract, checked by the
        // launcher) -- already in registers
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int f = (q >> 1) * CH_K + 16 * (q & 1) + 4 * grp, seg = 0;
            while (f >= F) { f -= F; ++seg; }
            int j = n;
#pragma unroll
            for (int k = 0; k < 8; ++k) j = seg == k + 1 ? nbj[k] : j;
            const bool ok = seg < segs && (seg == 0 || seg - 1 < xa.m_max) && j >= 0;
            eaw[q] = ok ? 1.0f : 0.0f;           // (applied behind the barrier: a multiply here would wait for every load above)
            ea[q] = *reinterpret_cast<const float4*>(obr + (ok ? j * F + f : 0));
        }
    }
    NMARL_STAMP(41)
    NMARL_STAGE_STORE(0)
    NMARL_STAMP(42)

    // ---- accumulators <- bias (+ zadd1 + zadd2);  C/D layout: col = lane & 15, row = 4 (lane >> 4) + reg
    f32x4 acc[16];
    float4 b4s[4];
    {
        const float* bn = a.bias + (int64_t)n * a.bias_sn;
        const float* z1 = MSG == 0 && a.zadd1 ? a.zadd1 + (int64_t)n * a.zadd1_sn : nullptr;
        const float* z2 = MSG == 0 && a.zadd2 ? a.zadd2 + (int64_t)n * a.zadd2_sn : nullptr;
        // column tile t = 4 gate + jj holds, for lane column c, UNIT 4 c + jj of that gate (the image permutes W's columns
        // accordingly): a lane's four jj values are four consecutive floats of a row -- inputs come in and results leave as
        // 16-byte accesses straight from / to the C/D layout, no LDS staging
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) b4s[g4] = *reinterpret_cast<const float4*>(bn + g4 * H + 4 * c);
        // (message kernels: the 64 accumulators are filled from these 16 registers only after the pre-phases -- the
        // pre-phases' operands are requested up front and need the room; they take no addends)
        if (MSG == 0) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc[4 * g4 + 0][r] = b4s[g4].x; acc[4 * g4 + 1][r] = b4s[g4].y; acc[4 * g4 + 2][r] = b4s[g4].z; acc[4 * g4 + 3][r] = b4s[g4].w;
                }
        }
        if (z1) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float4 v4 = *reinterpret_cast<const float4*>(z1 + rofs[r] * G4 + g4 * H + 4 * c);
                    acc[4 * g4 + 0][r] += v4.x; acc[4 * g4 + 1][r] += v4.y; acc[4 * g4 + 2][r] += v4.z; acc[4 * g4 + 3][r] += v4.w;
                }
        }
        if (z2) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float4 v4 = *reinterpret_cast<const float4*>(z2 + rofs[r] * G4 + g4 * H + 4 * c);
                    acc[4 * g4 + 0][r] += v4.x; acc[4 * g4 + 1][r] += v4.y; acc[4 * g4 + 2][r] += v4.z; acc[4 * g4 + 3][r] += v4.w;
                }
        }
    }
    float cp[4][4];
    {
        const float* cpn = a.c_prev + (int64_t)n * a.c_prev_sn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4 v4 = *reinterpret_cast<const float4*>(cpn + rofs[r] * H + 4 * c);
            cp[0][r] = v4.x; cp[1][r] = v4.y; cp[2][r] = v4.z; cp[3][r] = v4.w;
        }
    }
    {
        float4* d_ = reinterpret_cast<float4*>(lds + CH_FLOATS) + threadIdx.x;
        d_[0] = tg0; d_[512] = tg1; d_[1024] = tg2; d_[1536] = tg3; d_[2048] = tg4;
    }
    NMARL_STAMP(43)
    NMARL_STAMP(45)
    if (MSG != 0) {
        float4* d = reinterpret_cast<float4*>(m_lds);
        const int lim = xa.msg_kc * (CH_K * 64 / 4);
#pragma unroll
        for (int q = 0; q < MIQ; ++q) { const int i = threadIdx.x + 512 * q; if (i < lim) d[i] = mi[q]; }
    }
    NMARL_STAMP(46)
    if (ob_here) {
        float4* d = reinterpret_cast<float4*>(o_lds);
#pragma unroll
        for (int q = 0; q < 2; ++q) d[threadIdx.x + 512 * q] = oi[q];
    }
    if (HEAD == 2) {
        if (threadIdx.x < H) hw_lds[H * MAXA + MAXA + threadIdx.x] = hw2;
    } else if (HEAD != 0) {
        const int A = a.hd.A;
        hw_lds[threadIdx.x] = (int)(threadIdx.x & 7) < A ? hw0 : 0.0f;
        if (threadIdx.x < MAXA) hw_lds[H * MAXA + threadIdx.x] = (int)threadIdx.x < A ? hw1 : 0.0f;
        if (PV && threadIdx.x < H) hw_lds[H * MAXA + MAXA + threadIdx.x] = hw2;
    }
    // ENC: [6][64][4] W image + [128] biases -- behind the x slots; ENC_GLB: over the parked-cell-state slots behind the W_msg image
    // (6.5 of their 8 KB; the slots are first written after the message pre-phase, a block barrier behind the image's last read)
    float* e_lds = ENC_GLB ? m_lds + xa.msg_kc * (CH_K * 64) : hw_lds + HW_FLOATS + 8 * 512 * 4;
    // ENC 3 / 4: the W image (16 + 8 KB) borrows the x-slot region -- the slots are first written behind the pre-phase's own barrier,
    // when every wave has read its operands from the image; the biases sit behind the slots like the CACC forms'
    float* g_lds = hw_lds + HW_FLOATS;
    if constexpr (EGEN) {
#pragma unroll
        for (int q = 0; q < (EFP ? 12 : 8); ++q) g_lds[q * 512 + threadIdx.x] = ewt[q];
        if (threadIdx.x < (EFP ? 32 : 16)) *reinterpret_cast<float4*>(e_lds + 1536 + 4 * threadIdx.x) = float4{eacc[0][0], eacc[0][1], eacc[0][2], eacc[0][3]};
    } else if (ENC) {
        NMARL_STAMP(37)
#pragma unroll
        for (int q = 0; q < (EFP ? 3 : 2); ++q) e_lds[q * 512 + threadIdx.x] = ewt[q];
        if (threadIdx.x < (EFP ? 32 : 16)) *reinterpret_cast<float4*>(e_lds + 1536 + 4 * threadIdx.x) = float4{eacc[0][0], eacc[0][1], eacc[0][2], eacc[0][3]};
    }
    NMARL_STAMP(47)
    NMARL_STAGE_LOAD(nch > 2 ? 2 : nch - 1)
    __syncthreads();
    NMARL_STAMP(1)
    if (ENC) {
        // ---- ENC: operands from LDS, 24 MFMAs (k-step outer: four independent accumulators between two dependent ones), relu, park
        // in the lane's LDS slots, save for the update
        const int i16 = lane & 15;
        if constexpr (EGEN) {
            // ---- ENC 3 / 4: up to 16 + 8 k-steps, the k-step's weights from the borrowed x-slot region (uniform trip counts)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float4 b0 = *reinterpret_cast<const float4*>(e_lds + 1536 + 16 * mt + 4 * grp);
                eacc[mt] = f32x4{b0.x, b0.y, b0.z, b0.w};
                if constexpr (EFP) {
                    const float4 b1 = *reinterpret_cast<const float4*>(e_lds + 1536 + H + 16 * mt + 4 * grp);
                    eacc[4 + mt] = f32x4{b1.x, b1.y, b1.z, b1.w};
                }
            }
            const float4* gi_ = reinterpret_cast<const float4*>(g_lds) + lane;
            const int obk = (xa.e_ob_rows & 255) >> 2, fpk = (((xa.e_ob_rows >> 8) & 255) + 3) >> 2;
#pragma unroll
            for (int s_ = 0; s_ < 16; ++s_) {
                if (s_ < obk) {
                    const float4 w_ = gi_[s_ * 64];
                    eacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_.x, ein[s_], eacc[0], 0, 0, 0);
                    eacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_.y, ein[s_], eacc[1], 0, 0, 0);
                    eacc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_.z, ein[s_], eacc[2], 0, 0, 0);
                    eacc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_.w, ein[s_], eacc[3], 0, 0, 0);
                }
            }
            if constexpr (EFP) {
#pragma unroll
                for (int s_ = 0; s_ < 8; ++s_) {
                    if (s_ < fpk) {
                        const float4 w_ = gi_[(16 + s_) * 64];
                        eacc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_.x, ein[16 + s_], eacc[4], 0, 0, 0);
                        eacc[5] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_.y, ein[16 + s_], eacc[5], 0, 0, 0);
                        eacc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_.z, ein[16 + s_], eacc[6], 0, 0, 0);
                        eacc[7] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_.w, ein[16 + s_], eacc[7], 0, 0, 0);
                    }
                }
            }
            __syncthreads();                 // every wave has read the image: its LDS becomes the lane-private x slots
        } else {
        float4 w4[EFP ? 6 : 4];
#pragma unroll
        for (int s_ = 0; s_ < (EFP ? 6 : 4); ++s_) w4[s_] = reinterpret_cast<const float4*>(e_lds)[s_ * 64 + lane];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const float4 b0 = *reinterpret_cast<const float4*>(e_lds + 1536 + 16 * mt + 4 * grp);
            eacc[mt] = f32x4{b0.x, b0.y, b0.z, b0.w};
            if (EFP) {
                const float4 b1 = *reinterpret_cast<const float4*>(e_lds + 1536 + H + 16 * mt + 4 * grp);
                eacc[4 + mt] = f32x4{b1.x, b1.y, b1.z, b1.w};
            }
        }
        if (ENC_GLB) __syncthreads();        // every wave has read the image: its LDS becomes the parked-cell-state slots again
#pragma unroll
        for (int s_ = 0; s_ < 4; ++s_) {
            eacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s_].x, ein[s_], eacc[0], 0, 0, 0);
            eacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s_].y, ein[s_], eacc[1], 0, 0, 0);
            eacc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s_].z, ein[s_], eacc[2], 0, 0, 0);
            eacc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s_].w, ein[s_], eacc[3], 0, 0, 0);
        }
#pragma unroll
        for (int s_ = 4; s_ < (EFP ? 6 : 4); ++s_) {
            eacc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s_].x, ein[s_], eacc[4], 0, 0, 0);
            eacc[5] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s_].y, ein[s_], eacc[5], 0, 0, 0);
            eacc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s_].z, ein[s_], eacc[6], 0, 0, 0);
            eacc[7] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[s_].w, ein[s_], eacc[7], 0, 0, 0);
        }
        }
        NMARL_STAMP(50)
        unsigned pos = 0;                    // bit 4 mt + i: output 16 mt + 4 grp + i of row c is > 0 (the relu derivative the update needs)
        float* const so_ = ENC_GLB && e_out != nullptr ? e_out + (int64_t)n * e_out_sn + (row0 + c) * e_out_row + 4 * grp : nullptr;
#pragma unroll
        for (int mt = 0; mt < EMT; ++mt) {
            eacc[mt] = __builtin_elementwise_max(eacc[mt], f32x4{0.0f, 0.0f, 0.0f, 0.0f});
            const float4 v_ = float4{eacc[mt][0], eacc[mt][1], eacc[mt][2], eacc[mt][3]};
            if (ENC_LDS) xslot[512 * mt] = v_;                                   // (lane-private: re-read by this lane only)
            if (ENC_GLB && so_ != nullptr && row0 + c < a.E) *reinterpret_cast<float4*>(so_ + 16 * mt) = v_;     // columns 16 mt + 4 grp + {0..3}
#pragma unroll
            for (int i = 0; i < 4; ++i) pos |= (eacc[mt][i] > 0.0f ? 1u : 0u) << (4 * mt + i);
        }
        // one word per lane, 16 bytes per row: the update's encoder backward reads these instead of the 512-byte row of S
        if (e_bits != nullptr && row0 + c < a.E) e_bits[(int64_t)n * e_bits_sn + (row0 + c) * 4 + grp] = pos;
        NMARL_STAMP(51)
        if (ENC_LDS) {
            a0 = float4{eacc[0][0], eacc[0][1], eacc[0][2], eacc[0][3]};
            a1 = float4{eacc[1][0], eacc[1][1], eacc[1][2], eacc[1][3]};
        }
        // (ENC_LDS: the saved LSTM input of the update is NOT stored here: 8 x 16-byte stores per lane at once are a 16.8-MB burst from
        // all 256 blocks in the same phase, ~3.4 k cycles of blocked store issue in front of tick 0 (tools/step_timeline.py enc noout);
        // each x chunk's two pieces leave in the tick that multiplies them instead -- the A operands ARE those values.  ENC_GLB pays
        // that burst: it hides behind the message pre-phase that follows, whose operands were requested before the barrier)
        asm volatile("" :: "s"(ka_touch));
        NMARL_STAMP(38)
    }

    // one k-step of a 64-column product from an LDS image [k][c][4 t]: four MFMAs; a 32-row chunk of it: eight steps
#define NMARL_MSTEP(ACC, av, kl)                                                               \
        {                                                                                      \
            const float4 b_ = *reinterpret_cast<const float4*>(mb + (kl) * 64);                \
            ACC[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_.x, ACC[0], 0, 0, 0);          \
            ACC[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_.y, ACC[1], 0, 0, 0);          \
            ACC[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_.z, ACC[2], 0, 0, 0);          \
            ACC[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_.w, ACC[3], 0, 0, 0);          \
        }
#define NMARL_MCHUNK(ACC, IMG, kc, m0, m1)                                                     \
        {                                                                                      \
            const float* mb = (IMG) + (((kc) * CH_K + 4 * grp) * 16 + c) * 4;  /* + kl * 64 floats per k row */ \
            NMARL_MSTEP(ACC, m0.x, 0) NMARL_MSTEP(ACC, m0.y, 1) NMARL_MSTEP(ACC, m0.z, 2) NMARL_MSTEP(ACC, m0.w, 3)  \
            NMARL_MSTEP(ACC, m1.x, 16) NMARL_MSTEP(ACC, m1.y, 17) NMARL_MSTEP(ACC, m1.z, 18) NMARL_MSTEP(ACC, m1.w, 19) \
        }
    float4 encv[OBENC ? 4 : 1];                                      // the encoder's rows of this lane (C/D layout), for the pre-phase
    if (ob_here) {
        f32x4 eacc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) eacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) { ea[q].x *= eaw[q]; ea[q].y *= eaw[q]; ea[q].z *= eaw[q]; ea[q].w *= eaw[q]; }
        NMARL_MCHUNK(eacc, o_lds, 0, ea[0], ea[1])
        NMARL_MCHUNK(eacc, o_lds, 1, ea[2], ea[3])
        const float4 bo = bo4;
        float* eo = const_cast<float*>(xa.enc) + (int64_t)n * xa.enc_sn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4 v = float4{tanh_fast(eacc[0][r] + bo.x), tanh_fast(eacc[1][r] + bo.y), tanh_fast(eacc[2][r] + bo.z),
                                    tanh_fast(eacc[3][r] + bo.w)};
            if (row0 + 4 * grp + r < a.E) *reinterpret_cast<float4*>(eo + (row0 + 4 * grp + r) * xa.enc_row + 4 * c) = v;
            encv[r] = v;
        }
    }
    // The message pre-phase.  second_c = true_type: the VALUE re-step's message term (HEAD 4), from the neighbours' NEW h (h_new,
    // written through by their blocks earlier in this launch: L1-bypassing loads); nothing of it is kept.
    // msg_phase: U / W hold round 0 already (first phase: requested before the prologue's barrier)
    int grp_w = grp;                        // (the lane's row group as the tile WRITES address it: see CP_PARK behind the K loop)
    auto msg_phase = [&](auto second_c, float4 (&U)[16], float (&W)[4]) {
        constexpr bool SECOND = decltype(second_c)::value;
        constexpr bool reuse = !SECOND && carried;      // U[0..3] = the finished term of the lane's four rows
        f32x4 macc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) macc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        // one round of the gather forms: the four chunks of the two neighbour slots U / W hold = chunks KB .. KB + 3 of the message
        // input, against the 128 image rows resident in LDS
#define NMARL_MROUND(KB)                                                                       \
            _Pragma("unroll")                                                                  \
            for (int kc = 0; kc < 4; ++kc) {                                                   \
                if ((KB) + kc < xa.msg_kc) {                                                   \
                    const float w = W[kc >> 1];                                                \
                    float4 m0 = U[2 * kc], m1 = U[2 * kc + 1];                                 \
                    m0.x *= w; m0.y *= w; m0.z *= w; m0.w *= w; m1.x *= w; m1.y *= w; m1.z *= w; m1.w *= w; \
                    NMARL_MCHUNK(macc, m_lds, kc, m0, m1)                                      \
                }                                                                              \
            }
        if (reuse) {
        } else if (MSG != 2) {              // chunk kc = half (kc & 1) of neighbour slot (kc >> 1), K_m = 64 m_max <= 128 resident
            if constexpr (MSG_WIDE) {
                if (xa.msg_kc > 4) {
                    // lstm_comm with 3 or 4 neighbour slots (K_m = 192 / 256): two rounds of two slots into the same accumulators, chunks
                    // ascending.  The image does not fit LDS whole: rows 0..127 are resident (staged by the prologue), rows 128.. are REQUESTED
                    // here, in front of round 0's products, and stored over the first half once every wave of the block has read it.  A
                    // block-uniform branch (msg_kc is a launch argument); K_m = 192: the second half has 64 rows, nothing past the image is read.
                    const float4* g = reinterpret_cast<const float4*>(xa.msg_img + (int64_t)n * xa.msg_img_sn);
                    const int lim = xa.msg_kc * (CH_K * 64 / 4);                 // 3072 or 4096 float4 in all, 2048 of them resident
                    // (named registers: as an array living across the barriers it is demoted to scratch, like the staging registers)
                    const int i0 = 2048 + (int)threadIdx.x;
                    const float4 mw0 = g[i0], mw1 = g[i0 + 512], mw2 = g[i0 + 1024 < lim ? i0 + 1024 : 0], mw3 = g[i0 + 1536 < lim ? i0 + 1536 : 0];
                    NMARL_MROUND(0)
                    msg_load(second_c, K2{}, U, W);                              // slots 2 and 3 (absent: the own row, weight 0)
                    __syncthreads();                                             // the first half's last read
                    {
                        float4* d = reinterpret_cast<float4*>(m_lds) + threadIdx.x;
                        d[0] = mw0; d[512] = mw1;
                        if (i0 + 1024 < lim) { d[1024] = mw2; d[1536] = mw3; }       // (msg_kc 6: rows 192.. do not exist)
                    }
                    __syncthreads();
                    NMARL_MROUND(4)
                } else {
                    NMARL_MROUND(0)
                }
            } else {
                NMARL_MROUND(0)
            }
        } else {                            // mean over the existing neighbours (K_m = 64: two chunks), four neighbours per round
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) cnt += (k < xa.m_max && nbj[k] >= 0) ? 1 : 0;
            const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.0f;
            float4 sm[2][2];
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) sm[kc][0] = sm[kc][1] = float4{0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < xa.m_max; k0 += 4) {
                if (k0 > 0) msg_load(second_c, K4{}, U, W);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
                        for (int hh = 0; hh < 2; ++hh) {
                            const float4 u = U[4 * q + 2 * kc + hh];
                            sm[kc][hh].x += W[q] * u.x; sm[kc][hh].y += W[q] * u.y;
                            sm[kc][hh].z += W[q] * u.z; sm[kc][hh].w += W[q] * u.w;
                        }
            }
            if (SECOND) { NMARL_STAMP(52) }
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                float4 m0 = sm[kc][0], m1 = sm[kc][1];
                m0.x *= inv; m0.y *= inv; m0.z *= inv; m0.w *= inv; m1.x *= inv; m1.y *= inv; m1.z *= inv; m1.w *= inv;
                if (!SECOND && xa.mm_out && row0 + c < a.E) {        // (A layout: row c of the strip, k = 32 kc + 16 j + 4 grp + {0..3})
                    float* mo = xa.mm_out + (int64_t)n * xa.mm_sn + arow * xa.mm_row + kc * CH_K + 4 * grp;
                    *reinterpret_cast<float4*>(mo) = m0;
                    *reinterpret_cast<float4*>(mo + 16) = m1;
                }
                if (SECOND && CARRY != 0 && xa.mm_next) {          // = the next lock-step's mm_out rows (uniform base + 32-bit offsets: no address registers;
                    // rows past E fall outside the resource and are dropped)
                    const __amdgpu_buffer_rsrc_t rm_ = make_rsrc(xa.mm_next + (int64_t)n * xa.mm_next_sn, (uint32_t)(a.E * xa.mm_next_row * 4));
                    const uint32_t mo = row0 + c < a.E ? (uint32_t)(((row0 + c) * xa.mm_next_row + kc * CH_K + 4 * grp) * 4) : 0xfffffff0u;
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, m0), rm_, mo, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, m1), rm_, mo, 64, 0);
                }
                NMARL_MCHUNK(macc, m_lds, kc, m0, m1)
            }
        }
        if (SECOND) { NMARL_STAMP(53) }
        // result (C layout) + bias, relu / + enc -> the wave's LDS tile (A layout source) and, if asked, global memory
        const float* encn = MSG != 1 ? xa.enc + (int64_t)n * xa.enc_sn : nullptr;
        float* xo = (!SECOND && xa.xm_out) ? xa.xm_out + (int64_t)n * xa.xm_sn : nullptr;
        float* xo2 = (MSG == 3 && xa.xm2_out) ? xa.xm2_out + (int64_t)n * xa.xm2_sn : nullptr;
        const float4 bv = bv4;                                                    // tile t of lane column c = unit 4 c + t
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float4 v = float4{macc[0][r] + bv.x, macc[1][r] + bv.y, macc[2][r] + bv.z, macc[3][r] + bv.w};
            if (MSG != 2) {
                v.x = fmaxf(v.x, 0.0f); v.y = fmaxf(v.y, 0.0f); v.z = fmaxf(v.z, 0.0f); v.w = fmaxf(v.w, 0.0f);
            }
            if (reuse) v = U[r];
            if (SECOND && CARRY != 0 && xa.carry_out)          // (rows past E fall outside the resource and are dropped)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), make_rsrc(xa.carry_out + (int64_t)n * xa.carry_out_sn, (uint32_t)(a.E * (H * 4))),
                                                       (uint32_t)(((row0 + 4 * grp + r) * H + 4 * c) * 4), 0, 0);
            if (MSG == 3 && xo2 && row0 + 4 * grp + r < a.E)
                *reinterpret_cast<float4*>(xo2 + (row0 + 4 * grp + r) * xa.xm2_row + 4 * c) = v;
            if (MSG != 1) {
                float4 e4;
                if (OBENC && !SECOND && ob_here) {      // computed above: NOT re-read (the re-read was a memory round trip in front of the K loop
                    e4 = encv[r];                       // whose value was then thrown away -- round 6, tools/step_timeline.py 4 grid)
                } else if (HEAD == 4) {    // uniform base + a 32-bit offset made here: no row-address registers live across the launch (rofs dies early)
                    const uint32_t rr_ = row0 + 4 * grp + r < a.E ? (uint32_t)(row0 + 4 * grp + r) : (uint32_t)(a.E - 1);
                    e4 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(make_rsrc(encn, (uint32_t)(a.E * xa.enc_row * 4)),
                                                                                         (rr_ * (uint32_t)xa.enc_row + 4 * c) * 4, 0, 0));
                } else {
                    e4 = *reinterpret_cast<const float4*>(encn + rofs[r] * xa.enc_row + 4 * c);
                }
                v.x += e4.x; v.y += e4.y; v.z += e4.z; v.w += e4.w;
            }
            float* t_ = a_tile + (4 * grp_w + r) * APITCH + 4 * c;
            t_[0] = v.x; t_[1] = v.y; t_[2] = v.z; t_[3] = v.w;
            if (xo && row0 + 4 * grp + r < a.E) *reinterpret_cast<float4*>(xo + (row0 + 4 * grp + r) * xa.xm_row + 4 * c) = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    NMARL_STAMP(48)
    float keepr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) keepr[r] = 1.0f - a.done[rofs[r]];
    if (MSG != 0) {
        // chunk 0's A operands when they come from global memory (nx > 2: lstm_comm's [hx | hp] columns): requested BEFORE the
        // pre-phase, unconditionally (a valid dummy row otherwise), so their latency hides behind it
        const float* p0_ = nx > 2 ? xrow : hrow;
        a0 = *reinterpret_cast<const float4*>(p0_);
        a1 = *reinterpret_cast<const float4*>(p0_ + 16);
        msg_phase(std::false_type{}, PU, PW);
        if (nx <= 2) {                      // chunk 0 is a message chunk: from the wave's LDS tile
            const float* t_ = a_tile + c * APITCH + 4 * grp;
            a0.x = t_[0]; a0.y = t_[1]; a0.z = t_[2]; a0.w = t_[3];
            a1.x = t_[16]; a1.y = t_[17]; a1.z = t_[18]; a1.w = t_[19];
        }
    }
    NMARL_STAMP(49)
    if (MSG != 0) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[4 * g4 + 0][r] = b4s[g4].x; acc[4 * g4 + 1][r] = b4s[g4].y; acc[4 * g4 + 2][r] = b4s[g4].z; acc[4 * g4 + 3][r] = b4s[g4].w;
            }
    }

    // HEAD 4 with the lstm_ic3 message term: the whole LSTM input is message columns (KX = 64, the launcher insists), so the
    // re-step's kept x-side part is just the bias -- re-read it instead of holding 64 registers through the K loop
    constexpr bool ZS_BIAS = HEAD == 4 && MSG == 2;
    f32x4 zs[PV && !ZS_BIAS ? 16 : 1];
    // HEAD 4 with lstm_comm's message term: 256 VGPRs hold everything but one float4 through the K loop -- the previous cell state
    // of the lane's fourth row waits in a lane-private LDS slot behind the W_msg image (8 KB of the 9.7 KB left; it went to scratch)
    constexpr bool CP_PARK = HEAD == 4 && MSG == 1;
    float4* cp_park = reinterpret_cast<float4*>(m_lds + xa.msg_kc * (CH_K * 64)) + threadIdx.x;
    if (CP_PARK) *cp_park = float4{cp[0][3], cp[1][3], cp[2][3], cp[3][3]};
    NMARL_A_MASK(0, a0, a1)
    const int lag = DEPH ? (wave >> 2) : 0;      // wave group B computes chunk tau - 1 in tick tau
    if (DEPH && lag) __builtin_amdgcn_s_setprio(1);   // the lagging (younger) group wins issue arbitration: its MFMAs are
                                                      // what the other group's VALU epilogue has to hide behind
    int bsel = lag ? NBUF - 1 : 0;               // (tau - lag) mod NBUF, kept incrementally
    int wsel = 2 % NBUF;                         // (tau + 2) mod NBUF: the buffer chunk tau + 2 is staged into
    for (int tau = 0; tau < nch; ++tau) {
        // Loads are issued UNCONDITIONALLY (indices clamped): a load inside a branch makes the compiler's waitcnt pass
        // assume the worst path at the join and wait for everything in flight, i.e. expose the global latency of the
        // staging loads once per chunk.
        const int ch = tau - lag;                // -1 in group B's first tick (idle)
        const int chn = ch + 1 < nch ? ch + 1 : nch - 1;
        NMARL_A_LOAD(chn, n0, n1)
        if (ch >= 0) {
            if (!ZS_BIAS && ((HEAD == 3 && ch == nx) || (HEAD == 4 && ch == nx - 2))) {
                // x-side part complete: the value re-step adds the SAME addend (HEAD 4: all of it but the message columns)
#pragma unroll
                for (int t = 0; t < 16; ++t) zs[t] = acc[t];
            }
            NMARL_KCHUNK(lds + bsel * CH_FLOATS, a0, a1)
            if (ENC_LDS && ch < nx && e_out != nullptr && row0 + c < a.E) {      // ENC: this chunk of the encoded input, for the update
                float* so = e_out + (int64_t)n * e_out_sn + (row0 + c) * e_out_row + 4 * grp + ch * CH_K;
                *reinterpret_cast<float4*>(so) = a0;
                *reinterpret_cast<float4*>(so + 16) = a1;
            }
        }
        NMARL_STAMP(2 + 2 * tau)
        __syncthreads();                         // tick done: the oldest chunk's buffer is free, chunk tau + 1 visible
        NMARL_STAMP(3 + 2 * tau)
        if (tau + 2 < nch) NMARL_STAGE_STORE(wsel)
        const int chs = tau + 3 < nch ? tau + 3 : nch - 1;
        NMARL_STAGE_LOAD(chs)
        a0 = n0; a1 = n1;
        NMARL_A_MASK(chn, a0, a1)
        bsel = bsel + 1 == NBUF ? 0 : bsel + 1;
        wsel = wsel + 1 == NBUF ? 0 : wsel + 1;
    }
    if (DEPH && lag) {                           // group B's last chunk, while group A is already in its epilogue
        if (HEAD == 3 && nch - 1 == nx) {
#pragma unroll
            for (int t = 0; t < 16; ++t) zs[t] = acc[t];
        }
        NMARL_KCHUNK(lds + bsel * CH_FLOATS, a0, a1)
    }
    NMARL_STAMP(20)
    if (CP_PARK) {
        const float4 v = *cp_park;
        cp[0][3] = v.x; cp[1][3] = v.y; cp[2][3] = v.z; cp[3][3] = v.w;
        int l_ = threadIdx.x;                    // the tile addresses behind the loop are formed again from the thread index (kept
        asm volatile("" : "+v"(l_));             // across it, one went to scratch)
        grp_w = (l_ & 63) >> 4;
    }
    if (nxt_here) {                              // (after the last tick's barrier: the W_msg image is dead)
        float4* d = reinterpret_cast<float4*>(m_lds);
        d[threadIdx.x] = nfa; d[threadIdx.x + 512] = nfb;
    }
    const unsigned epoch = HEAD == 4 ? (unsigned)__builtin_amdgcn_readfirstlane((int)epoch_raw) + 1u : 0u;
    bool early_ok = false;                       // HEAD 4: the re-step's neighbour rows were requested behind flags that were up
    // ENC + env step: what the hand-off word of this lane's replica held before this agent's add (lanes 0..15), the lane's own
    // draw, and the strip's env state as requested right behind the draw
    unsigned ev_old = 0;
    int ev_act = -1;
    float ev_h[2] = {0.f, 0.f}, ev_v[2] = {0.f, 0.f}, ev_v0[2] = {0.f, 0.f};
    int ev_t[2] = {0, 0}, ev_c[2] = {0, 0};

    // ---- lane-local cell epilogue.  A lane holds units 4 c .. 4 c + 3 of rows 4 grp + r (column permutation of the image):
    // every output leaves as 16-byte stores of contiguous row pieces, 256 B per row and instruction.  (4-byte stores in the
    // natural C/D layout were issue-bound, ~10 k cycles per wave; staging through LDS cost ~7 k.)
    float* gn = a.gates ? a.gates + (int64_t)n * a.gates_sn : nullptr;
    float* cn = a.c_new + (int64_t)n * a.c_new_sn;
    float* hn_out = a.h_new + (int64_t)n * a.h_new_sn;
    float hv_[4][4];
    const f32x4 keepv = f32x4{keepr[0], keepr[1], keepr[2], keepr[3]};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const f32x4 gi = sigm4(acc[0 + jj]), gf = sigm4(acc[4 + jj]), go = sigm4(acc[8 + jj]), gu = tanh4(acc[12 + jj]);
        const f32x4 cpv = f32x4{cp[jj][0], cp[jj][1], cp[jj][2], cp[jj][3]};
        const f32x4 cv = gf * (cpv * keepv) + gi * gu;
        const f32x4 hv = go * tanh4(cv);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (HEAD != 0) a_tile[(4 * grp_w + r) * APITCH + 4 * c + jj] = hv[r];   // K loop done: the tile is free
            cp[jj][r] = cv[r];                                                     // c' (HEAD 3 / 4: the re-step's previous cell)
            hv_[jj][r] = hv[r];
        }
        acc[0 + jj] = gi; acc[4 + jj] = gf; acc[8 + jj] = go; acc[12 + jj] = gu;
    }
    {
        // HEAD 4: h' is written THROUGH (sc1) -- the neighbours' blocks read it later in this launch (offset in a VGPR) -- FIRST, and
        // published at once (the four stores drained, one flag per (agent, block, wave)): the neighbours' re-steps wait for these
        // rows, not for this wave's gates, cell state or actor head, which all follow
        if (HEAD == 4) {
            const __amdgpu_buffer_rsrc_t rh_ = make_rsrc(hn_out, (uint32_t)(a.E * (H * 4)));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + 4 * grp + r;
                if (row < a.E)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, float4{hv_[0][r], hv_[1][r], hv_[2][r], hv_[3][r]}), rh_,
                                                           (uint32_t)((row * H + 4 * c) * 4), 0, SC1);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0 && !(xa.fault && blockIdx.x == 0))
                __hip_atomic_store((gu32*)(xa.sync + 16) + ((n * a.blocks_per_agent + blk_u) * WAVES2 + wave), epoch, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            NMARL_STAMP(26)
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = row0 + 4 * grp + r;
            if (row < a.E) {
                *reinterpret_cast<float4*>(cn + row * H + 4 * c) = float4{cp[0][r], cp[1][r], cp[2][r], cp[3][r]};
                const float4 h4 = float4{hv_[0][r], hv_[1][r], hv_[2][r], hv_[3][r]};
                if (HEAD != 4)
                    *reinterpret_cast<float4*>(hn_out + row * H + 4 * c) = h4;
                if (gn) {
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4)
                        *reinterpret_cast<float4*>(gn + row * G4 + g4 * H + 4 * c) =
                            float4{acc[4 * g4 + 0][r], acc[4 * g4 + 1][r], acc[4 * g4 + 2][r], acc[4 * g4 + 3][r]};
                }
            }
        }
    }
    NMARL_STAMP(21)
    if (HEAD != 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int act_l = -1;
        if (HEAD == 2) head_epilogue<2>(a, n, xa.N, row0, lane, a_tile, hw_lds + H * MAXA + MAXA);
        else act_l = head_policy_lds(a, n, xa.N, row0, lane, a_tile, hw_lds, hw_lds + H * MAXA);
        if (GENV && xa.gv_on && act_l >= 0 && !(xa.fault && blockIdx.x == 0)) {     // (test hook: block 0's actions never arrive either)
            // the drawn action of (replica row0 + lane, agent n) -> the replica's hand-off word (no return value: nothing here waits)
            typedef __attribute__((address_space(1))) unsigned long long gu64;
            const int hi_ = n >= 13 ? 1 : 0;
            __hip_atomic_fetch_add((gu64*)xa.gv_words + 2 * (row0 + lane) + hi_,
                                   ((unsigned long long)act_l << (3 * (n - 13 * hi_))) | (1ull << 59), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (ENC && !EGEN && xa.ev_on) {
            // ---- ENV (1/2): every drawn action goes into its replica's hand-off word by ONE atomic add -- 2 bits of payload per agent
            // + an arrival count above them -- whose return value is looked at after the value re-step (which hides the trip): the
            // lane that finds N - 1 earlier arrivals holds all N actions of that replica.  The strip's env state (16 replicas x 8
            // vehicles: two (replica, vehicle) pairs per lane) is requested here as well, by every wave.
            if (act_l >= 0)
                ev_old = __hip_atomic_fetch_add((gu32*)xa.ev_cnt + (row0 + lane), ((unsigned)act_l << (2 * n)) | 0x10000u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
            ev_act = act_l;
            const int64_t n_lanes = a.E * nmarl_cacc::N;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int64_t gq = row0 * nmarl_cacc::N + q * NMARL_WAVE + lane;
                const int64_t gc = gq < n_lanes ? gq : n_lanes - 1;
                ev_h[q] = xa.ev_h[gc]; ev_v[q] = xa.ev_v[gc];
                ev_t[q] = xa.ev_t[gc >> 3]; ev_c[q] = xa.ev_coll[gc >> 3]; ev_v0[q] = xa.ev_v0[gc >> 3];
            }
        }
    }
    NMARL_STAMP(22)
    if (nxt_here) {
        // ---- msg' = relu(h' W_mfc + b): h' is in the wave's tile (A layout source), the image in LDS behind this barrier
        __syncthreads();
        f32x4 facc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) facc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            const float* t_ = a_tile + c * APITCH + kc * CH_K + 4 * grp;
            const float4 m0 = float4{t_[0], t_[1], t_[2], t_[3]};
            const float4 m1 = float4{t_[16], t_[17], t_[18], t_[19]};
            NMARL_MCHUNK(facc, m_lds, kc, m0, m1)
        }
        float* no = xa.nxt_out + (int64_t)n * xa.nxt_out_sn;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (row0 + 4 * grp + r < a.E)
                *reinterpret_cast<float4*>(no + (row0 + 4 * grp + r) * H + 4 * c) =
                    float4{fmaxf(facc[0][r] + nb4.x, 0.0f), fmaxf(facc[1][r] + nb4.y, 0.0f), fmaxf(facc[2][r] + nb4.z, 0.0f),
                           fmaxf(facc[3][r] + nb4.w, 0.0f)};
    }
    if (HEAD == 4) {
        // (this wave's rows were published behind the cell epilogue's first stores, in front of the actor head)
        gu32* flags = (gu32*)(xa.sync + 16);
        const int bpa = a.blocks_per_agent, blk = blk_u;
        // ---- one LOOK at the neighbours' flags (no waiting): blocks run in step, so their same-numbered waves have usually published
        // by now -- then the rows requested here are the new h and fly under the h part of the re-step, whose MFMAs need no vector
        // memory.  The request is UNCONDITIONAL (a load inside a branch costs a conservative wait at the join): rows read too early
        // are simply requested again behind the blocking poll below.
        {
            // (lane k looks at neighbour k's flag: ONE memory round trip for all of them, a ballot decides)
            int jl = -1;
#pragma unroll
            for (int k = 0; k < 8; ++k) jl = lane == k ? nbj[k] : jl;
            const bool watch = lane < xa.m_max && lane < 8 && jl >= 0;
            const unsigned v = __hip_atomic_load(flags + (((watch ? jl : n) * bpa + blk) * WAVES2 + wave), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool up = __ballot(watch && v != epoch) == 0ull;
            early_ok = up;
            NMARL_NOTE(54, up ? 1 : 2)
            asm volatile("" ::: "memory");               // the payload loads stay below the look
            msg_load(std::true_type{}, K0{}, PU, PW);
        }
        NMARL_STAMP(31)
    }
    if (PV) {
        // ---- the value re-step (quirk Q1): z = x-side addend + (h' keep) @ Wh from the two resident Wh chunks
        if (ZS_BIAS) {
            const float* bn = a.bias + (int64_t)n * a.bias_sn;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const float4 b4 = *reinterpret_cast<const float4*>(bn + g4 * H + 4 * c);
#pragma unroll
                for (int r = 0; r < 4; ++r) { acc[4 * g4 + 0][r] = b4.x; acc[4 * g4 + 1][r] = b4.y; acc[4 * g4 + 2][r] = b4.z; acc[4 * g4 + 3][r] = b4.w; }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 16; ++t) acc[t] = zs[t];
        }
#pragma unroll
        for (int hc = 0; hc < 2; ++hc) {
            const float* ar = a_tile + c * APITCH + hc * CH_K + 4 * grp;
            float4 r0, r1;
            r0.x = ar[0] * keepA; r0.y = ar[1] * keepA; r0.z = ar[2] * keepA; r0.w = ar[3] * keepA;
            r1.x = ar[16] * keepA; r1.y = ar[17] * keepA; r1.z = ar[18] * keepA; r1.w = ar[19] * keepA;
            NMARL_KCHUNK(lds + ((nx + hc) % NBUF) * CH_FLOATS, r0, r1)
        }
        NMARL_STAMP(23)
        __builtin_amdgcn_wave_barrier();                 // every lane has read its A operands: the tile may be overwritten
        if (HEAD == 4) {
            // ---- the message columns of the re-step: from the neighbours' NEW h, published by the same wave of their blocks
            gu32* flags = (gu32*)(xa.sync + 16);
            const int bpa = a.blocks_per_agent, blk = blk_u;
            bool give_up = false;
            if (!early_ok) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int j = nbj[k];
                    if (k >= xa.m_max || j < 0 || give_up) continue;
                    gu32* f = flags + ((j * bpa + blk) * WAVES2 + wave);
                    for (unsigned spins = 0;; ++spins) {
                        const unsigned v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                        if (v == epoch) break;
                        if (spins > xa.max_spins) {           // a neighbour's block is not running: not co-resident (see the launcher)
                            if (lane == 0) {                  // sticky: the optimiser step refuses this batch (nmarl_rmsprop_tf_clip_guarded)
                                __hip_atomic_store((gu32*)xa.sync + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (xa.status) __hip_atomic_store((gu32*)xa.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                            give_up = true;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
                }
                asm volatile("" ::: "memory");               // the payload loads stay below the polls
                msg_load(std::true_type{}, K0{}, PU, PW);
            }
            NMARL_STAMP(27)
            // the W chunks of the message columns: requested here, in flight during the message term, stored behind its barrier
            NMARL_STAGE_LOAD(nx - 2)
            {
                const float4* g_ = img + (int64_t)(nx - 1) * (CH_FLOATS / 4) + threadIdx.x;
                tg0 = g_[0]; tg1 = g_[512]; tg2 = g_[1024]; tg3 = g_[1536]; tg4 = g_[2048];
            }
            msg_phase(std::true_type{}, PU, PW);         // -> the wave's A tile
            NMARL_STAMP(28)
            __syncthreads();                             // every wave is through with the Wh chunks
            NMARL_STAGE_STORE(0)
            {
                float4* d_ = reinterpret_cast<float4*>(lds + CH_FLOATS) + threadIdx.x;
                d_[0] = tg0; d_[512] = tg1; d_[1024] = tg2; d_[1536] = tg3; d_[2048] = tg4;
            }
            __syncthreads();
            NMARL_STAMP(29)
#pragma unroll
            for (int mc = 0; mc < 2; ++mc) {
                const float* buf = lds + mc * CH_FLOATS + (4 * grp * 16 + c) * 20;
                const float* ar = a_tile + c * APITCH + mc * CH_K + 4 * grp;
                float4 r0, r1;
                r0.x = ar[0]; r0.y = ar[1]; r0.z = ar[2]; r0.w = ar[3];
                r1.x = ar[16]; r1.y = ar[17]; r1.z = ar[18]; r1.w = ar[19];
                NMARL_CHUNK(buf, r0, r1)
            }
            NMARL_STAMP(30)
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const f32x4 gi = sigm4(acc[0 + jj]), gf = sigm4(acc[4 + jj]), go = sigm4(acc[8 + jj]), gu = tanh4(acc[12 + jj]);
            const f32x4 cpv = f32x4{cp[jj][0], cp[jj][1], cp[jj][2], cp[jj][3]};
            const f32x4 cv = gf * (cpv * keepv) + gi * gu;
            const f32x4 hv = go * tanh4(cv);
#pragma unroll
            for (int r = 0; r < 4; ++r) a_tile[(4 * grp_w + r) * APITCH + 4 * c + jj] = hv[r];
        }
        NMARL_STAMP(33)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        NMARL_STAMP(24)
        head_epilogue<3>(a, n, xa.N, row0, lane, a_tile, hw_lds + H * MAXA + MAXA);
        NMARL_STAMP(25)
        if (ENC && !EGEN && xa.ev_on) {
            // ---- ENV (2/2): envs/cacc_env.py:191-242 for the replicas whose LAST arrival this wave was (on average 2 of its 16).
            // The word's return value carries the other agents' draws, so nothing is read back and no wave ever waits for
            // another: no co-residency requirement, no failure mode, no memory-ordering argument beyond the atomic itself.  The
            // replicas are packed eight to a pass (one per aligned 8-lane group, lane = 8 k + vehicle), their state comes out of
            // the prefetched registers by cross-lane reads; state, reward and the compact observation of lock-step t + 1 are plain
            // stores (their reader is the next launch), the word is left zero for the next launch.  cacc_step_group = the env
            // kernels' arithmetic, operation for operation.
            const bool last_l = ev_act >= 0 && (ev_old >> 16) == (unsigned)(xa.N - 1);
            const unsigned pay_l = (ev_old | ((unsigned)(ev_act < 0 ? 0 : ev_act) << (2 * n))) & 0xffffu;
            if (last_l) xa.ev_cnt[row0 + lane] = 0u;
            unsigned long long todo = __ballot(last_l);                  // (uniform: bits 0..15)
            while (todo) {
                int rsel = -1;                                           // the row of this lane's group: the (lane >> 3)-th set bit
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int rk = todo ? (int)__builtin_ctzll(todo) : -1;
                    todo = todo ? (todo & (todo - 1)) : 0ull;
                    rsel = (lane >> 3) == k ? rk : rsel;
                }
                const bool valid = rsel >= 0;
                const int rr = valid ? rsel : 0;
                const int av = lane & 7;
                const int q = rr * nmarl_cacc::N + av;                   // the pair's place among the strip's 128: lane q & 63, slot q >> 6
                const unsigned pay = (unsigned)__shfl((int)pay_l, rr, NMARL_WAVE);
                const float h0 = __shfl(ev_h[0], q & 63, NMARL_WAVE), h1 = __shfl(ev_h[1], q & 63, NMARL_WAVE);
                const float v0 = __shfl(ev_v[0], q & 63, NMARL_WAVE), v1 = __shfl(ev_v[1], q & 63, NMARL_WAVE);
                const float w0 = __shfl(ev_v0[0], q & 63, NMARL_WAVE), w1 = __shfl(ev_v0[1], q & 63, NMARL_WAVE);
                const int t0 = __shfl(ev_t[0], q & 63, NMARL_WAVE), t1 = __shfl(ev_t[1], q & 63, NMARL_WAVE);
                const int c0 = __shfl(ev_c[0], q & 63, NMARL_WAVE), c1 = __shfl(ev_c[1], q & 63, NMARL_WAVE);
                const bool hi = q >= NMARL_WAVE;
                int64_t e = row0 + rr;
                e = e < a.E ? e : a.E - 1;
                nmarl_cacc::cacc_step_group(xa.ev_p, e, av, valid, hi ? h1 : h0, hi ? v1 : v0, (int)((pay >> (2 * av)) & 3u), hi ? t1 : t0,
                                            (hi ? c1 : c0) != 0, hi ? w1 : w0, xa.ev_h, xa.ev_v, xa.ev_u, xa.ev_t, xa.ev_coll, xa.ev_v0,
                                            xa.ev_obs, xa.ev_rew, xa.ev_done, xa.ev_grew, xa.ev_auto_reset, xa.ev_seed, xa.ev_base,
                                            xa.ev_episode);
            }
            NMARL_STAMP(39)
        }
        if (HEAD == 4) {
            // the last BLOCK of the launch to get here starts the next generation: no flag of this one is read any more
            // (one counter update per block: same-address atomics serialise, 2048 of them cost the last waves ~8 us)
            __syncthreads();
            if (threadIdx.x == 0) {
                gu32* sy = (gu32*)xa.sync;
                const unsigned old = __hip_atomic_fetch_add(sy + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (old == n_lstm - 1) {
                    __hip_atomic_store(sy + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(sy, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
#undef NMARL_MCHUNK
#undef NMARL_MSTEP
#undef NMARL_STAGE_LOAD
#undef NMARL_STAGE_STORE
#undef NMARL_A_LOAD
#undef NMARL_A_MASK
#undef NMARL_KCHUNK
}

// image[n][ch][kl][c][t] = W[32 ch + kl][64 (t >> 2) + 4 c + (t & 3)] (t < 16; 16..19 = 0), W = [wx (KX rows); wh (64 rows)]:
// tile t = 4 gate + jj of lane column c is unit 4 c + jj of that gate (see the kernel's epilogue)
__global__ void lstm_wimage_kernel(const int N, const int KX, const float* wx, const int64_t wx_sn, const float* wh,
                                   const int64_t wh_sn, float* img, const int64_t img_sn) {
    const int per_agent = (KX + H) * 320;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * per_agent) return;
    const int n = (int)(i / per_agent), o = (int)(i % per_agent);
    const int k = o / 320, cc = (o % 320) / 20, t = o % 20;
    float v = 0.0f;
    const int col = (t >> 2) * H + 4 * cc + (t & 3);
    if (t < 16) v = k < KX ? wx[(int64_t)n * wx_sn + (int64_t)k * G4 + col] : wh[(int64_t)n * wh_sn + (int64_t)(k - KX) * G4 + col];
    img[(int64_t)n * img_sn + o] = v;
}

// bf16x3 image: the fp32 image's chunks (same bytes per k row), each in the layout of chunk_bf16x3 -- dword
// (16 grp + c) X3_PITCH + 8 t + 4 h + jp of chunk ch packs elements j = 2 jp, 2 jp + 1 (low half first) of the hi (h = 0) or
// lo (h = 1) fragment of W[32 ch + kr(j)][64 (t >> 2) + 4 c + (t & 3)], kr(j) = 4 grp + j (j < 4), 16 + 4 grp + j - 4; the
// rest of the chunk is 0.  hi = bf16_rne(w), lo = bf16_rne(w - hi) by plain casts (NaN stays NaN).
__global__ void lstm_wimage_bf16x3_kernel(const int N, const int KX, const float* wx, const int64_t wx_sn, const float* wh,
                                          const int64_t wh_sn, unsigned* img, const int64_t img_sn) {
    const int per_agent = (KX + H) * 320;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * per_agent) return;
    const int n = (int)(i / per_agent), o = (int)(i % per_agent);
    const int ch = o / CH_FLOATS, r = o % CH_FLOATS;
    const int gc = r / X3_PITCH, q = r % X3_PITCH;
    unsigned v = 0u;
    if (gc < 64 && q < 128) {
        const int grp = gc >> 4, cc = gc & 15, t = q >> 3, hl = (q >> 2) & 1, jp = q & 3;
        const int col = (t >> 2) * H + 4 * cc + (t & 3);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = 2 * jp + e;
            const int k = ch * CH_K + (j < 4 ? 4 * grp + j : 16 + 4 * grp + j - 4);
            const float w = k < KX ? wx[(int64_t)n * wx_sn + (int64_t)k * G4 + col] : wh[(int64_t)n * wh_sn + (int64_t)(k - KX) * G4 + col];
            const __bf16 hb = (__bf16)w;
            const __bf16 b = hl ? (__bf16)(w - (float)hb) : hb;
            v |= (unsigned)__builtin_bit_cast(unsigned short, b) << (16 * e);
        }
    }
    img[(int64_t)n * img_sn + o] = v;
}

// msg image[k][c][t] = W_msg[k][4 c + t]  (K_m rows, 64 columns): a lane fetches the B operands of the 4 column tiles of
// one k with a single ds_read_b128
__global__ void lstm_msg_wimage_kernel(const int N, const int K, const float* w, const int64_t w_sn, float* img,
                                       const int64_t img_sn) {
    const int per_agent = K * 64;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * per_agent) return;
    const int n = (int)(i / per_agent), o = (int)(i % per_agent);
    const int k = o / 64, cc = (o % 64) / 4, t = o % 4;
    img[(int64_t)n * img_sn + o] = w[(int64_t)n * w_sn + (int64_t)k * 64 + 4 * cc + t];
}

inline bool stride_ok(int64_t s, int64_t need) { return s >= need && (s % 4) == 0; }

}  // namespace

extern "C" int nmarl_lstm_wimage_floats(int32_t KX) { return (KX + H) * 320; }

extern "C" int nmarl_lstm_step_sync_words(int64_t E, int32_t N) {
    return (int)(16 + (int64_t)N * ((E + ROWS_B - 1) / ROWS_B) * WAVES2);
}

extern "C" int nmarl_lstm_wimage(int32_t N, int32_t KX, const float* wx, int64_t wx_sn, const float* wh, int64_t wh_sn,
                                 float* img, int64_t img_sn, int32_t precision, void* stream) {
    if (N <= 0 || KX < 0 || KX > MAX_KX || KX % CH_K || !wh || !img || (KX > 0 && !wx) || img_sn < (int64_t)(KX + H) * 320 ||
        (img_sn % 4) || ((uintptr_t)img % 16) || wh_sn < H * G4 || (KX > 0 && wx_sn < (int64_t)KX * G4) || precision < 0 || precision > 1)
        return NMARL_EINVAL;
    const int64_t total = (int64_t)N * (KX + H) * 320;
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (precision)
        hipLaunchKernelGGL(lstm_wimage_bf16x3_kernel, grid, dim3(256), 0, st, N, KX, wx, wx_sn, wh, wh_sn, reinterpret_cast<unsigned*>(img), img_sn);
    else
        hipLaunchKernelGGL(lstm_wimage_kernel, grid, dim3(256), 0, st, N, KX, wx, wx_sn, wh, wh_sn, img, img_sn);
    return nmarl_check_launch();
}

extern "C" int nmarl_lstm_msg_wimage(int32_t N, int32_t K, const float* w_msg, int64_t w_sn, float* img, int64_t img_sn,
                                     void* stream) {
    if (N <= 0 || K <= 0 || K % CH_K || K > 256 || !w_msg || !img || w_sn < (int64_t)K * 64 || img_sn < (int64_t)K * 64 ||
        (img_sn % 4) || ((uintptr_t)img % 16))
        return NMARL_EINVAL;
    const int64_t total = (int64_t)N * K * 64;
    hipLaunchKernelGGL(lstm_msg_wimage_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       N, K, w_msg, w_sn, img, img_sn);
    return nmarl_check_launch();
}

// ---- in-launch hand-off: residency and the test hook
int nmarl_handoff_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return -1;
    if (const char* e = getenv("NMARL_TEST_FAKE_CUS")) {
        const int v = atoi(e);
        if (v > 0) cus = v;
    }
    return cus;
}

static std::atomic<int> g_fault_in{0};
extern "C" int nmarl_test_handoff_fault(int32_t nth) {
    if (nth < 0) return NMARL_EINVAL;
    g_fault_in.store(nth);
    return NMARL_OK;
}
bool nmarl_handoff_take_fault() {
    int v = g_fault_in.load();
    while (v > 0 && !g_fault_in.compare_exchange_weak(v, v - 1)) {}
    return v == 1;
}

NMARL_INTERNAL int nmarl_bptt_coupled_occupancy(int K);      // lstm_bptt.hip: blocks per CU of the coupled BPTT kernel
NMARL_INTERNAL int nmarl_bptt_dial_occupancy(int K);         // lstm_bptt.hip: ... of its lstm_dial instantiations

extern "C" int nmarl_handoff_capacity(int32_t which, int32_t K) {
    const int cus = nmarl_handoff_cus();
    if (cus < 0 || K <= 0) return -1;
    int per_cu = 0;
    if (which == 1) {
        // the lock-step kernel with a message term (HEAD 4): two chunk buffers + tiles + head weights + the message image (+ the
        // observation encoder's image where it can exist, lstm_ic3: K = 64)
        if (K % CH_K || K > 128) return -1;
        const size_t lb = (size_t)(LDSX_FLOATS + K * 64 + (K == H ? H * 64 : 0)) * sizeof(float) + (K == H ? 0 : 512 * sizeof(float4));   // (<4,1>: + its parked cell-state slots)
        const int lb_max = (int)((LDSX_FLOATS + CH_FLOATS) * sizeof(float));
        // the instantiation that will be launched: K = 64 is lstm_ic3's <4,2> (different registers / LDS: the encoder image), else
        // lstm_comm's <4,1>; queried once per (device, kind) and kept -- the launch path asks for it at every lock-step
        static std::atomic<int> cache[64][2];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return -1;
        const int kd = K == H ? 1 : 0;
        const int hit = (dev >= 0 && dev < 64) ? cache[dev][kd].load() : 0;
        if (hit > 0) {
            per_cu = hit - 1;
        } else {
            const void* fn = K == H ? reinterpret_cast<const void*>(lstm_step_x_kernel<4, 2>) : reinterpret_cast<const void*>(lstm_step_x_kernel<4, 1>);
            hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lb_max);
            if (rc == hipSuccess)
                rc = K == H ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lstm_step_x_kernel<4, 2>, 512, lb)
                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lstm_step_x_kernel<4, 1>, 512, lb);
            if (rc != hipSuccess) return -1;
            if (dev >= 0 && dev < 64) cache[dev][kd].store(per_cu + 1);
        }
    } else if (which == 2) {
        per_cu = nmarl_bptt_coupled_occupancy(K);
        if (per_cu < 0) return -1;
    } else if (which == 3) {
        per_cu = nmarl_bptt_dial_occupancy(K);
        if (per_cu < 0) return -1;
    } else {
        return -1;
    }
    return per_cu * cus;
}

extern "C" int nmarl_lstm_step_grid_env_blocks(int64_t E, int32_t N);

extern "C" int nmarl_lstm_step_x(const nmarl_step_x_t* s, void* stream) {
    if (!s) return NMARL_EINVAL;
    const int64_t E = s->E;
    const int32_t N = s->N, KX = s->KX, KX2 = s->KX2, prec = s->precision;
    const float *x = s->x, *x2 = s->x2, *h_in = s->h_in, *img = s->img, *bias = s->bias, *zadd1 = s->zadd1, *zadd2 = s->zadd2,
                *c_prev = s->c_prev, *done = s->done;
    float *gates = s->gates, *c_new = s->c_new, *h_new = s->h_new;
    const int64_t x_sn = s->x_sn, x_row = s->x_row, x2_sn = s->x2_sn, x2_row = s->x2_row, h_sn = s->h_sn, img_sn = s->img_sn,
                  bias_sn = s->bias_sn, zadd1_sn = s->zadd1_sn, zadd2_sn = s->zadd2_sn, c_prev_sn = s->c_prev_sn, gates_sn = s->gates_sn,
                  c_new_sn = s->c_new_sn, h_new_sn = s->h_new_sn;
    const nmarl_head_t* head = s->head;
    const nmarl_msg_t* msg = s->msg;
    const nmarl_step_enc_t* enc = s->enc;
    const nmarl_grid_env_t* genv = s->genv;
    const int mk = msg ? msg->kind : 0;
    const int kind = head ? head->kind : 0;
    // which optional parts go together: a message term needs a head and takes no addends; the in-launch encoders and the grid env
    // role need head kind 3; the encoders write x with message kind 1 and read no x without a message term; the grid role needs
    // message kind 2; bf16x3: the MSG = 0 forms
    if ((msg && (mk == 0 || kind == 0 || zadd1 || zadd2)) || ((enc || genv) && kind != 3) || (enc && (mk > 1 || (mk == 1) != !!x)) ||
        (genv && mk != 2) || prec < 0 || prec > 1 || (prec && (msg || genv)))
        return NMARL_EINVAL;
    const int KM = mk ? H : 0;                   // columns of x the message pre-phase produces
    if (s->H != H || E < 0 || N <= 0 || KX < 0 || KX > MAX_KX || KX % CH_K || KX2 < 0 || KX2 > KX || KX2 % CH_K || mk < 0 || mk > 3 ||
        (mk && (KX2 != 0 || KX < H)) ||
        (E > 0 && (!h_in || !img || !bias || !c_prev || !done || !c_new || !h_new || (KX - KX2 - KM > 0 && !x && (!enc || mk)) || (KX2 > 0 && !x2))))
        return NMARL_EINVAL;
    if (mk && E > 0) {
        if (msg->m_max <= 0 || msg->m_max > 8 || !msg->nbr_idx || !msg->img || !msg->b || msg->b_sn < H ||
            msg->K != (mk == 2 ? H : H * msg->m_max) || msg->K > ((mk == 1 && (kind == 1 || kind == 2)) ? 256 : 128) || msg->img_sn < (int64_t)msg->K * 64 || (msg->img_sn % 4) ||
            ((uintptr_t)msg->img % 16) || ((uintptr_t)msg->b % 16) || (msg->b_sn % 4) ||
            (mk != 1 && (!msg->enc || msg->enc_row < H || msg->enc_sn < E * msg->enc_row || ((uintptr_t)msg->enc % 16) ||
                         (msg->enc_row % 4) || (msg->enc_sn % 4))) ||
            (msg->out && (msg->out_row < H || msg->out_sn < E * msg->out_row || ((uintptr_t)msg->out % 16) || (msg->out_row % 4) ||
                          (msg->out_sn % 4))) ||
            (mk == 3 && (KX != H || !msg->src || msg->src_sn < E * (int64_t)H || (msg->src_sn % 4) || ((uintptr_t)msg->src % 16) ||
                         (msg->out2 && (msg->out2_row < H || msg->out2_sn < E * msg->out2_row || ((uintptr_t)msg->out2 % 16) ||
                                        (msg->out2_row % 4) || (msg->out2_sn % 4))))))
            return NMARL_EINVAL;
    }
    if (kind < 0 || kind > 3 || (mk == 3 && kind == 3)) return NMARL_EINVAL;     // lstm_dial: the two-launch lock-step only
    if (kind != 0 && E > 0) {
        if (head->A <= 0 || head->A > MAXA || !head->w || !head->b || head->b_sn < (kind == 2 ? 1 : head->A)) return NMARL_EINVAL;
        if ((kind == 1 || kind == 3) && (head->w_sn < (int64_t)H * head->A || !head->pi_out || head->pi_sn < E * head->A || !head->act_out ||
                          head->mode < 0 || head->mode > 2 || (head->mode == 0 && !head->u)))
            return NMARL_EINVAL;
        if (kind == 3 && (!head->w2 || !head->b2 || head->w2_sn < H || head->b2_sn < 1 || !head->v_out || head->v_sn < E))
            return NMARL_EINVAL;
        if (kind == 2 && (head->m_max < 0 || head->w_sn < H + (int64_t)head->m_max * head->A || !head->v_out || head->v_sn < E ||
                          (head->m_max > 0 && (!head->act_in || !head->nbr_idx))))
            return NMARL_EINVAL;
    }
    if (E == 0) return NMARL_OK;
    if (!stride_ok(h_sn, E * H) || !stride_ok(bias_sn, G4) || (zadd1 && !stride_ok(zadd1_sn, E * G4)) ||
        (zadd2 && !stride_ok(zadd2_sn, E * G4)) || !stride_ok(c_prev_sn, E * H) || !stride_ok(c_new_sn, E * H) ||
        !stride_ok(h_new_sn, E * H) || (gates && !stride_ok(gates_sn, E * G4)) || ((uintptr_t)h_in % 16) || ((uintptr_t)img % 16) ||
        ((uintptr_t)c_new % 16) || ((uintptr_t)h_new % 16) || (gates && ((uintptr_t)gates % 16)) ||
        ((uintptr_t)bias % 16) || ((uintptr_t)c_prev % 16) || (zadd1 && ((uintptr_t)zadd1 % 16)) || (zadd2 && ((uintptr_t)zadd2 % 16)) ||
        img_sn < (int64_t)(KX + H) * 320 || (img_sn % 4) ||
        (KX - KX2 - KM > 0 && (!enc || mk) && (x_row < KX - KX2 - KM || (x_row % 4) || (x_sn % 4) || ((uintptr_t)x % 16))) ||
        (KX2 > 0 && (x2_row < KX2 || (x2_row % 4) || (x2_sn % 4) || ((uintptr_t)x2 % 16))))
        return NMARL_EINVAL;
    XArgs xa{};
    FusedArgs& a = xa.f;
    a.h_in = h_in; a.bias = bias; a.zadd1 = zadd1; a.zadd2 = zadd2; a.c_prev = c_prev; a.done = done;
    a.gates = gates; a.c_new = c_new; a.h_new = h_new;
    a.h_sn = h_sn; a.bias_sn = bias_sn; a.zadd1_sn = zadd1_sn; a.zadd2_sn = zadd2_sn;
    a.c_prev_sn = c_prev_sn; a.gates_sn = gates_sn; a.c_new_sn = c_new_sn; a.h_new_sn = h_new_sn;
    a.E = E;
    a.blocks_per_agent = (int)((E + ROWS_B - 1) / ROWS_B);
    if (kind != 0) a.hd = *head;
    // (ENC with a message term: the encoders' output travels THROUGH x -- the S slot of the saved activations -- so x stays)
    xa.x = (KX - KX2 - KM > 0 && (!enc || mk)) ? x : nullptr; xa.x_sn = x_sn; xa.x_row = x_row;
    xa.x2 = KX2 > 0 ? x2 : nullptr; xa.x2_sn = x2_sn; xa.x2_row = x2_row;
    xa.img = img; xa.img_sn = img_sn;
    xa.nx = KX / CH_K; xa.nx1 = (KX - KX2) / CH_K; xa.N = N;
    if (mk) {
        xa.msg_kc = msg->K / CH_K; xa.m_max = msg->m_max; xa.nbr_idx = msg->nbr_idx; xa.msg_img = msg->img;
        xa.msg_img_sn = msg->img_sn; xa.msg_b = msg->b; xa.msg_b_sn = msg->b_sn; xa.enc = msg->enc; xa.enc_sn = msg->enc_sn;
        xa.enc_row = msg->enc_row; xa.xm_out = msg->out; xa.xm_sn = msg->out_sn; xa.xm_row = msg->out_row;
        if (mk == 2 && msg->mean_out) {
            if (msg->mean_out_row < H || msg->mean_out_sn < E * msg->mean_out_row || ((uintptr_t)msg->mean_out % 16) || (msg->mean_out_row % 4) ||
                (msg->mean_out_sn % 4))
                return NMARL_EINVAL;
            xa.mm_out = msg->mean_out; xa.mm_sn = msg->mean_out_sn; xa.mm_row = msg->mean_out_row;
        }
        if (msg->carry_in || msg->carry_out || msg->mean_next) {
            if (kind != 3 || mk == 3 || (msg->carry_in && (msg->carry_in_sn < E * (int64_t)H || (msg->carry_in_sn % 4) || ((uintptr_t)msg->carry_in % 16))) ||
                (msg->carry_out && (msg->carry_out_sn < E * (int64_t)H || (msg->carry_out_sn % 4) || ((uintptr_t)msg->carry_out % 16))) ||
                (msg->mean_next && (mk != 2 || msg->mean_next_row < H || msg->mean_next_sn < E * msg->mean_next_row || ((uintptr_t)msg->mean_next % 16) ||
                                    (msg->mean_next_row % 4) || (msg->mean_next_sn % 4))))
                return NMARL_EINVAL;
            xa.carry_in = msg->carry_in; xa.carry_in_sn = msg->carry_in_sn; xa.carry_out = msg->carry_out; xa.carry_out_sn = msg->carry_out_sn;
            xa.mm_next = msg->mean_next; xa.mm_next_sn = msg->mean_next_sn; xa.mm_next_row = msg->mean_next_row;
        }
        if (mk == 3) {
            xa.src = msg->src; xa.src_sn = msg->src_sn; xa.xm2_out = msg->out2; xa.xm2_sn = msg->out2_sn; xa.xm2_row = msg->out2_row;
            if (msg->next_out) {
                if (kind != 1 || !msg->next_img || !msg->next_b || msg->next_img_sn < H * 64 || (msg->next_img_sn % 4) ||
                    ((uintptr_t)msg->next_img % 16) || msg->next_b_sn < H || (msg->next_b_sn % 4) || ((uintptr_t)msg->next_b % 16) ||
                    msg->next_out_sn < E * (int64_t)H || (msg->next_out_sn % 4) || ((uintptr_t)msg->next_out % 16))
                    return NMARL_EINVAL;
                xa.nxt_img = msg->next_img; xa.nxt_img_sn = msg->next_img_sn; xa.nxt_b = msg->next_b; xa.nxt_b_sn = msg->next_b_sn;
                xa.nxt_out = msg->next_out; xa.nxt_out_sn = msg->next_out_sn;
            }
        }
    }
    static NmarlPerDeviceOnce lds_once;
    // no message pre-phase: three chunk buffers (de-phased wave groups); with it: two + the W_msg image
    const int lb_max = (int)((LDSX_FLOATS + CH_FLOATS) * sizeof(float));
    // (lstm_comm with K > 128, head kinds 1 / 2: 128 rows of the W_msg image are resident at a time, the second half streams in)
    const size_t lb = (size_t)(LDSX_FLOATS + (mk ? (msg->K < 128 ? msg->K : 128) * 64 : CH_FLOATS)) * sizeof(float);
    if (const unsigned long long lds_bit = lds_once.pending(); lds_bit != ~0ull) {
#define NMARL_SET_LDS(k) \
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lb_max) != hipSuccess) return NMARL_EHIP;
        NMARL_SET_LDS((lstm_step_x_kernel<0, 0>)) NMARL_SET_LDS((lstm_step_x_kernel<1, 0>)) NMARL_SET_LDS((lstm_step_x_kernel<2, 0>))
        NMARL_SET_LDS((lstm_step_x_kernel<3, 0>)) NMARL_SET_LDS((lstm_step_x_kernel<1, 1>)) NMARL_SET_LDS((lstm_step_x_kernel<2, 1>))
        NMARL_SET_LDS((lstm_step_x_kernel<1, 2>)) NMARL_SET_LDS((lstm_step_x_kernel<2, 2>))
        NMARL_SET_LDS((lstm_step_x_kernel<1, 3>)) NMARL_SET_LDS((lstm_step_x_kernel<2, 3>))
        NMARL_SET_LDS((lstm_step_x_kernel<4, 1>)) NMARL_SET_LDS((lstm_step_x_kernel<4, 2>)) NMARL_SET_LDS((lstm_step_x_kernel<4, 1, 1>))
        NMARL_SET_LDS((lstm_step_x_kernel<4, 1, 0, 1>)) NMARL_SET_LDS((lstm_step_x_kernel<4, 2, 0, 1>)) NMARL_SET_LDS((lstm_step_x_kernel<4, 1, 1, 1>))
        NMARL_SET_LDS((lstm_step_x_kernel<4, 1, 0, 2>)) NMARL_SET_LDS((lstm_step_x_kernel<4, 2, 0, 2>)) NMARL_SET_LDS((lstm_step_x_kernel<4, 1, 1, 2>))
        NMARL_SET_LDS((lstm_step_x_kernel<0, 0, 0, 0, 1>)) NMARL_SET_LDS((lstm_step_x_kernel<1, 0, 0, 0, 1>))
        NMARL_SET_LDS((lstm_step_x_kernel<2, 0, 0, 0, 1>)) NMARL_SET_LDS((lstm_step_x_kernel<3, 0, 0, 0, 1>))
#undef NMARL_SET_LDS
        lds_once.done(lds_bit);
    }
    dim3 grid(a.blocks_per_agent * N);
    if (enc && enc->F != 5) {
        // the input encoders on a GENERAL input layout (ENC 3: both, ENC 4: the observation encoder alone): F own features (a multiple
        // of 4) x (1 + m_max) observation slots <= 64 inputs, A <= 8 fingerprint entries x m_max neighbours <= 32 inputs, m_max <= 4;
        // the uncoupled nets' policy + value step, fp32, no env step inside (the ATSC grid: F = 12, m_max = 4, A = 5)
        const bool single = !enc->w_fp;
        const int F = enc->F, A = enc->A, mm = enc->m_max;
        if (mk != 0 || prec || enc->env || F <= 0 || (F % 4) || mm < 0 || mm > 4 || F * (1 + mm) > H || N > 32 ||
            KX != (single ? H : 2 * H) || KX2 != 0 || zadd1 || zadd2 ||
            (!single && (A <= 0 || A > MAXA || mm < 1 || A * mm > 32)))
            return NMARL_EINVAL;
        const int ob_rows = F * (1 + mm), fp_rows = single ? 0 : A * mm;
        if (!enc->ob || !enc->w_ob || !enc->b_ob || enc->ob_row < (int64_t)N * F || enc->w_ob_sn < (int64_t)ob_rows * H || enc->b_ob_sn < H ||
            (enc->b_ob_sn % 4) || ((uintptr_t)enc->b_ob % 16) ||
            (!single && (!enc->fp || !enc->b_fp || enc->fp_sn < E * A || enc->w_fp_sn < (int64_t)fp_rows * H || enc->b_fp_sn < H ||
                         (enc->b_fp_sn % 4) || ((uintptr_t)enc->b_fp % 16))) ||
            (enc->out && (((uintptr_t)enc->out % 16) || enc->out_row < (single ? H : 2 * H) || (enc->out_row % 4) || (enc->out_sn % 4) ||
                          enc->out_sn < E * enc->out_row)) ||
            (enc->relu_bits && (single || ((uintptr_t)enc->relu_bits % 4) || enc->relu_bits_sn < E * 4)))
            return NMARL_EINVAL;
        for (int i = 0; i < N * mm; ++i)                           // nbr: [N][m_max], -1 padded
            if (enc->nbr[i] < -1 || enc->nbr[i] >= N) return NMARL_EINVAL;
        xa.e_ob = enc->ob; xa.e_ob_row = enc->ob_row; xa.e_fp = enc->fp; xa.e_fp_sn = enc->fp_sn;
        xa.e_wob = enc->w_ob; xa.e_bob = enc->b_ob; xa.e_wfp = enc->w_fp; xa.e_bfp = enc->b_fp;
        xa.e_wob_sn = enc->w_ob_sn; xa.e_bob_sn = enc->b_ob_sn; xa.e_wfp_sn = enc->w_fp_sn; xa.e_bfp_sn = enc->b_fp_sn;
        xa.e_out = enc->out; xa.e_out_sn = enc->out_sn; xa.e_out_row = enc->out_row;
        xa.e_bits = enc->relu_bits; xa.e_bits_sn = enc->relu_bits_sn;
        for (int i = 0; i < 64; ++i) {                             // agent i's four slots as signed bytes (see XArgs)
            unsigned w = 0;
            for (int k = 0; k < 4; ++k) w |= (unsigned)((i < N && k < mm ? enc->nbr[i * mm + k] : -1) & 255) << (8 * k);
            xa.e_nbr[i] = (int)w;
        }
        xa.ob_F = F; xa.e_ob_rows = ob_rows | (fp_rows << 8) | ((single ? 1 : A) << 16);
        // same LDS as the CACC forms: the 16 + 8 KB weight image borrows the x-slot region until the pre-phase's barrier
        const size_t lb_g = (size_t)(2 * CH_FLOATS + HW_FLOATS + 8 * 512 * 4 + 6 * 64 * 4 + 2 * H) * sizeof(float);
        static NmarlPerDeviceOnce gen_once;
        if (const unsigned long long bit = gen_once.pending(); bit != ~0ull) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_step_x_kernel<3, 0, 3>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lb_g) != hipSuccess ||
                hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_step_x_kernel<3, 0, 4>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lb_g) != hipSuccess)
                return NMARL_EHIP;
            gen_once.done(bit);
        }
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (single) hipLaunchKernelGGL((lstm_step_x_kernel<3, 0, 4>), grid, dim3(512), lb_g, st, xa);
        else hipLaunchKernelGGL((lstm_step_x_kernel<3, 0, 3>), grid, dim3(512), lb_g, st, xa);
        return nmarl_check_launch();
    }
    if (enc) {
        // the input encoders inside the launch (ENC 1) on the CACC input layout: the uncoupled nets' policy + value step (<3,0,1>), or
        // NeurComm's one-launch lock-step (<4,1,1>: x = the S slot the encoders' [hx | hp] goes to AND the K loop reads it back from)
        const bool coupled = mk == 1 && kind == 3;
        const bool single = !enc->w_fp;                        // ENC 2: the observation encoder alone (IA2C; ConseNet with m_max = 0)
        const int ob_rows = 5 * (1 + enc->m_max);
        if ((mk != 0 && !coupled) || KX != (coupled ? 3 * H : single ? H : 2 * H) || KX2 != 0 || zadd1 || zadd2 || N > 32 || enc->F != 5 ||
            (coupled && single) || (single ? (enc->m_max != 0 && enc->m_max != 2) : (enc->A != 4 || enc->m_max != 2)) ||
            !enc->ob || !enc->w_ob || !enc->b_ob || enc->ob_row < (int64_t)N * 5 || enc->w_ob_sn < (int64_t)ob_rows * H || enc->b_ob_sn < H ||
            (enc->b_ob_sn % 4) || ((uintptr_t)enc->b_ob % 16) ||
            (!single && (!enc->fp || !enc->b_fp || enc->fp_sn < E * 4 || enc->w_fp_sn < 8 * H || enc->b_fp_sn < H || (enc->b_fp_sn % 4) ||
                         ((uintptr_t)enc->b_fp % 16))) ||
            (enc->out && (((uintptr_t)enc->out % 16) || enc->out_row < (single ? H : 2 * H) || (enc->out_row % 4) || (enc->out_sn % 4) ||
                          enc->out_sn < E * enc->out_row)) ||
            (coupled && enc->out && (enc->out != x || enc->out_sn != x_sn || enc->out_row != x_row)))
            return NMARL_EINVAL;
        for (int i = 0; i < 2 * N; ++i)
            if (enc->nbr[i] < -1 || enc->nbr[i] >= N) return NMARL_EINVAL;
        xa.e_ob = enc->ob; xa.e_ob_row = enc->ob_row; xa.e_fp = enc->fp; xa.e_fp_sn = enc->fp_sn;
        xa.e_wob = enc->w_ob; xa.e_bob = enc->b_ob; xa.e_wfp = enc->w_fp; xa.e_bfp = enc->b_fp;
        xa.e_wob_sn = enc->w_ob_sn; xa.e_bob_sn = enc->b_ob_sn; xa.e_wfp_sn = enc->w_fp_sn; xa.e_bfp_sn = enc->b_fp_sn;
        xa.e_out = enc->out; xa.e_out_sn = enc->out_sn; xa.e_out_row = enc->out_row;
        if (coupled) { xa.e_out = const_cast<float*>(x); xa.e_out_sn = x_sn; xa.e_out_row = x_row; }
        if (enc->relu_bits && (((uintptr_t)enc->relu_bits % 4) || enc->relu_bits_sn < E * 4)) return NMARL_EINVAL;
        xa.e_bits = enc->relu_bits; xa.e_bits_sn = enc->relu_bits_sn;
        for (int i = 0; i < 64; ++i) xa.e_nbr[i] = (i < 2 * N && enc->m_max == 2) ? enc->nbr[i] : -1;
        xa.e_ob_rows = ob_rows;
        if (single && enc->relu_bits) return NMARL_EINVAL;       // (the sign image is the two-layer encoding's: nmarl_fc_bwd_pair)
        if (enc->env) {
            // the CACC env step of this lock-step behind the action draw (ENV block of the kernel)
            const nmarl_cacc_params_t* p = enc->env;
            if (N != NMARL_CACC_N || head->A > 4 || !p->compact_obs || p->T <= 0 || p->batch_size <= 0 || (p->scenario != 0 && p->scenario != 1) || p->dt <= 0.f ||
                p->h_g <= p->h_s || p->u_max == 0.f || p->v_star == 0.f || p->h_star == 0.f || !enc->h || !enc->v || !enc->u || !enc->t ||
                !enc->collided || !enc->v0_init || !enc->obs_out || !enc->reward || !enc->done || !enc->global_reward ||
                !enc->cnt || ((uintptr_t)enc->cnt % 4) || ((uintptr_t)enc->obs_out % 16) || (enc->auto_reset && !enc->episode) ||
                head->act_out == nullptr)
                return NMARL_EINVAL;
            xa.ev_on = 1; xa.ev_auto_reset = enc->auto_reset ? 1 : 0; xa.ev_p = *p;
            xa.ev_h = enc->h; xa.ev_v = enc->v; xa.ev_u = enc->u; xa.ev_t = enc->t; xa.ev_coll = enc->collided; xa.ev_v0 = enc->v0_init;
            xa.ev_obs = enc->obs_out; xa.ev_rew = enc->reward; xa.ev_done = enc->done; xa.ev_grew = enc->global_reward;
            xa.ev_seed = enc->seed; xa.ev_base = enc->env_id_base; xa.ev_episode = enc->episode;
            xa.ev_cnt = enc->cnt;
        }
        if (!coupled) {
            static NmarlPerDeviceOnce enc_once;
            const size_t lb_e = (size_t)(2 * CH_FLOATS + HW_FLOATS + 8 * 512 * 4 + 6 * 64 * 4 + 2 * H) * sizeof(float);
            if (const unsigned long long bit = enc_once.pending(); bit != ~0ull) {
                if (hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_step_x_kernel<3, 0, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lb_e) != hipSuccess ||
                    hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_step_x_kernel<3, 0, 2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lb_e) != hipSuccess ||
                    hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_step_x_kernel<3, 0, 1, 0, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lb_e) != hipSuccess ||
                    hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_step_x_kernel<3, 0, 2, 0, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lb_e) != hipSuccess)
                    return NMARL_EHIP;
                enc_once.done(bit);
            }
            hipStream_t st = static_cast<hipStream_t>(stream);
            if (prec) {
                if (single) hipLaunchKernelGGL((lstm_step_x_kernel<3, 0, 2, 0, 1>), grid, dim3(512), lb_e, st, xa);
                else hipLaunchKernelGGL((lstm_step_x_kernel<3, 0, 1, 0, 1>), grid, dim3(512), lb_e, st, xa);
            } else if (single) hipLaunchKernelGGL((lstm_step_x_kernel<3, 0, 2>), grid, dim3(512), lb_e, st, xa);
            else hipLaunchKernelGGL((lstm_step_x_kernel<3, 0, 1>), grid, dim3(512), lb_e, st, xa);
            return nmarl_check_launch();
        }
    }
    if (mk && kind == 3) {
        // policy step + value re-step of a coupled net in ONE launch: the re-step's message term needs the neighbours' new h, handed
        // over between blocks inside the launch -- every block must be resident (one block per CU: 512 threads, > 80 KB LDS)
        const int cap = nmarl_handoff_capacity(1, msg->K);
        if (cap < 0) return NMARL_EHIP;
        if (!msg->sync || ((uintptr_t)msg->sync % 4) || ((uintptr_t)msg->status % 4) || (int)grid.x > cap ||
            E * (int64_t)(H * 4) >= (int64_t)1 << 32 || (mk == 2 && (KX != H || E * msg->enc_row * 4 >= (int64_t)1 << 32)))
            return NMARL_EINVAL;
        xa.sync = msg->sync;
        xa.status = msg->status;
        xa.fault = nmarl_handoff_take_fault() ? 1 : 0;
        xa.max_spins = xa.fault ? NMARL_HANDOFF_FAULT_SPINS : NMARL_HANDOFF_MAX_SPINS;
        if (genv) {
            // the synthetic grid's env step as a role of this launch: the compute units the LSTM blocks leave idle run it
            const nmarl_grid_params_t* gp = genv->params;
            const int env_blocks = nmarl_lstm_step_grid_env_blocks(E, N);
            if (!gp || env_blocks <= 0 || N != NMARL_GRID_N || head->A > 7 || !msg->ob || !gp->compact_obs || gp->objective != 0 || gp->T <= 0 ||
                gp->norm_wave <= 0.f || !genv->q || !genv->transit || !genv->prev_action || !genv->t || !genv->xi || !genv->obs_out ||
                !genv->reward || !genv->done || !genv->global_reward || !genv->words || ((uintptr_t)genv->words % 8) ||
                ((uintptr_t)genv->obs_out % 16) || ((uintptr_t)genv->q % 16) || ((uintptr_t)genv->transit % 16) ||
                (genv->auto_reset && !genv->episode) || !msg->status)
                return NMARL_EINVAL;
            xa.gv_on = 1; xa.gv_lstm_blocks = (int)grid.x; xa.gv_auto_reset = genv->auto_reset ? 1 : 0; xa.gv_p = *gp;
            xa.gv_q = genv->q; xa.gv_tr = genv->transit; xa.gv_prev = genv->prev_action; xa.gv_t = genv->t; xa.gv_xi = genv->xi;
            xa.gv_obs = genv->obs_out; xa.gv_rew = genv->reward; xa.gv_done = genv->done; xa.gv_grew = genv->global_reward;
            xa.gv_seed = genv->seed; xa.gv_base = genv->env_id_base; xa.gv_episode = genv->episode;
            xa.gv_words = reinterpret_cast<unsigned long long*>(genv->words);
            grid = dim3(grid.x + env_blocks);
        }
    }
    size_t lb_extra = 0;
    if (msg && msg->ob) {
        // in-kernel observation encoder: the one-launch lstm_ic3 step only; compact observation, 16-byte pieces
        // (the kernel takes the slot owners from nbr_idx: ob_nbr must be [own index | nbr_idx row], i.e. ob_segs = m_max + 1)
        if (mk != 2 || kind != 3 || msg->ob_F <= 0 || (msg->ob_F % 4) || msg->ob_segs != msg->m_max + 1 || msg->ob_F * msg->ob_segs > H ||
            !msg->ob_nbr || !msg->ob_img || !msg->ob_b || ((uintptr_t)msg->ob % 16) || (msg->ob_row % 4) ||
            msg->ob_row < (int64_t)N * msg->ob_F || ((uintptr_t)msg->ob_img % 16) || msg->ob_img_sn < H * 64 || (msg->ob_img_sn % 4) ||
            ((uintptr_t)msg->ob_b % 16) || (msg->ob_b_sn % 4) || msg->ob_b_sn < H)
            return NMARL_EINVAL;
        xa.ob = msg->ob; xa.ob_row = msg->ob_row; xa.ob_F = msg->ob_F; xa.ob_segs = msg->ob_segs; xa.ob_nbr = msg->ob_nbr;
        xa.ob_img = msg->ob_img; xa.ob_img_sn = msg->ob_img_sn; xa.ob_b = msg->ob_b; xa.ob_b_sn = msg->ob_b_sn;
        lb_extra = (size_t)H * 64 * sizeof(float);
    }
    if (mk == 1 || mk == 2) {
        // the pre-phase gathers OTHER agents' previous h while their blocks write h_new: no panel of h_new may overlap a
        // panel of h_in (in-place stepping is for nets without the in-kernel message term; lstm_dial's pre-phase reads the
        // message vectors instead, which no block of this launch writes)
        const int64_t span = E * (int64_t)H;
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                const float* a0 = h_in + i * h_sn;
                const float* b0 = h_new + j * h_new_sn;
                if (a0 < b0 + span && b0 < a0 + span) return NMARL_EINVAL;
            }
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mk == 1 && kind == 3) lb_extra += 512 * sizeof(float4);      // HEAD 4 / MSG 1: the parked cell-state slots (CP_PARK)
#define NMARL_LX(HD, MS)                                                                                                         \
    if (prec) hipLaunchKernelGGL((lstm_step_x_kernel<HD, 0, 0, 0, 1>), grid, dim3(512), lb + lb_extra, st, xa);                 \
    else hipLaunchKernelGGL((lstm_step_x_kernel<HD, MS>), grid, dim3(512), lb + lb_extra, st, xa)
    // the one-launch lock-steps: by what the caller hands on between them (nmarl_msg_t carry_in / carry_out / mean_next)
    const int carry = !msg ? 0 : msg->carry_in ? 2 : (msg->carry_out || msg->mean_next) ? 1 : 0;
#define NMARL_LC(MS, EN)                                                                                                         \
    if (carry == 2) hipLaunchKernelGGL((lstm_step_x_kernel<4, MS, EN, 2>), grid, dim3(512), lb + lb_extra, st, xa);              \
    else if (carry == 1) hipLaunchKernelGGL((lstm_step_x_kernel<4, MS, EN, 1>), grid, dim3(512), lb + lb_extra, st, xa);         \
    else hipLaunchKernelGGL((lstm_step_x_kernel<4, MS, EN, 0>), grid, dim3(512), lb + lb_extra, st, xa);
    if (mk == 0) {
        if (kind == 0) NMARL_LX(0, 0); else if (kind == 1) NMARL_LX(1, 0); else if (kind == 2) NMARL_LX(2, 0); else NMARL_LX(3, 0);
    } else if (mk == 1) {
        if (kind == 1) NMARL_LX(1, 1); else if (kind == 2) NMARL_LX(2, 1);
        else if (enc) { NMARL_LC(1, 1) }
        else { NMARL_LC(1, 0) }
    } else if (mk == 2) {
        if (kind == 1) NMARL_LX(1, 2); else if (kind == 2) NMARL_LX(2, 2); else { NMARL_LC(2, 0) }
    } else {
        if (kind == 1) NMARL_LX(1, 3); else NMARL_LX(2, 3);
    }
#undef NMARL_LX
#undef NMARL_LC
    return nmarl_check_launch();
}

// env-role blocks a grid launch gets: the compute units the LSTM blocks leave idle, at most one per group of 16 replicas
extern "C" int nmarl_lstm_step_grid_env_blocks(int64_t E, int32_t N) {
    if (E <= 0 || N <= 0) return 0;
    const int cap = nmarl_handoff_capacity(1, H);
    const int64_t lstm = (int64_t)N * ((E + ROWS_B - 1) / ROWS_B), groups = (E + 15) / 16;
    if (cap <= 0 || lstm >= cap) return 0;
    const int64_t room = cap - lstm;
    return (int)(room < groups ? room : groups);
}

extern "C" int nmarl_lstm_step_grid_words(int64_t E) { return E <= 0 ? 0 : (int)(2 * E); }

extern "C" int nmarl_lstm_step_env_words(int64_t E) { return E <= 0 ? 0 : (int)((E + 63) / 64 * 64); }

#ifdef NMARL_STEP_TIMELINE
extern "C" int nmarl_timeline_set(unsigned long long* p, void* stream) {
    hipLaunchKernelGGL(timeline_set_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), p);
    return nmarl_check_launch();
}
#endif
