// EXL3 trellis encoder (quantize_tiles) for gfx950: the tail-biting Viterbi search that turns a 256-weight tile into 256 16-bit trellis
// states.  Semantics: exllamav3_ext/quant/quantize.cu:27-87 and quant/quantize_tiles_kernel.cuh (restated in tests/_trellis_encoder_ref.py);
// design and measurements: DESIGN.md 4.12.  One translation unit per bits-per-weight K (-DG2_K=K), the codebook a template argument.
//
// Trellis: E = 65536 >> K nodes (the low 16-K bits of a state).  Node e at position t has 2^K candidate states s_k = (k << (16-K)) | e,
// whose predecessor node is p_k = s_k >> K = (k << (16-2K)) | (e >> K).  Step cost, fp16 RN at every operation:
//   d = decode(s_k); delta = d - w[t]; c = delta*delta (first position of a pass) or fma(delta, delta, C_prev[p_k]); C[e] = min over k,
// strictly-less so the smallest k wins ties.
//
// Layout.  One workgroup per tile, NT = min(1024, E/2) threads; thread j owns the node pairs (2p, 2p+1), p = j + NT*i, i < NI = E/(2 NT).
// Both nodes of a pair share every predecessor, so one LDS read of C_prev[p_k] feeds a packed-fp16 fma for two nodes.  The two cost
// arrays (2 x E fp16 = 128 KiB at K = 1) live in LDS for every K.  A node's back-pointer is its winning k (K bits: p_k follows from (k, e));
// thread j packs the 2K-bit pair codes of its NI pairs into one 32- or 16-bit word per position, stored to the caller's workspace at
// word[t][j] (coalesced).  The min over k is ONE v_min_u32 per node: costs are >= 0 so their fp16 bit patterns order as unsigned
// integers, and (cost << 16) | k orders by cost, then by k.
#include "exl3_common.cuh"
#include "exl3_api_internal.h"

#ifndef G2_K
#error "compile with -DG2_K=<bits per weight>"
#endif

namespace {

constexpr int qt_nt(int K) { return (65536 >> K) / 2 < 1024 ? (65536 >> K) / 2 : 1024; }
constexpr int qt_ni(int K) { return (65536 >> K) / 2 / qt_nt(K); }
constexpr int qt_word_bytes(int K) { return qt_ni(K) * 2 * K > 16 ? 4 : 2; }
// occupancy the register budget is cut for: K = 1 holds one workgroup per CU (128 KiB of costs, 16 waves = 4 per SIMD); every other K fills the
// CU's 32 wave slots (8 per SIMD, <= 64 VGPRs)
constexpr int qt_waves_per_simd(int K) { return K == 1 ? 4 : 8; }

template <int CB> constexpr uint32_t qt_mult() { return CB == EXL3_CB_3INST ? 89226354u : (CB == EXL3_CB_MCG ? 0xCBAC1FEDu : 0x83DCD12Du); }

// decode of the two states whose codebook products are pr0 (low half) and pr1 (high half); one RN fp16 op per value, as decode_exact
template <int CB>
__device__ __forceinline__ half2_t qt_decode2(uint32_t pr0, uint32_t pr1)
{
    if constexpr (CB != EXL3_CB_MUL1)
    {
        uint32_t x0 = cb_mask3inst(pr0), x1 = cb_mask3inst(pr1);
        half2_t lo = u32_as_half2(__builtin_amdgcn_perm(x1, x0, 0x05040100u));      // (lo16(x0), lo16(x1))
        half2_t hi = u32_as_half2(__builtin_amdgcn_perm(x1, x0, 0x07060302u));      // (hi16(x0), hi16(x1))
        return lo + hi;                                                              // v_pk_add_f16
    }
    else
    {
        uint32_t b0 = __builtin_amdgcn_sad_u8(pr0, 0u, 0x6400u), b1 = __builtin_amdgcn_sad_u8(pr1, 0u, 0x6400u);
        half2_t h = u32_as_half2(__builtin_amdgcn_perm(b1, b0, 0x05040100u));
        const half2_t k_inv = u32_as_half2(0x1eee1eeeu), k_bias = u32_as_half2(0xc931c931u);
        return __builtin_elementwise_fma(h, k_inv, k_bias);                          // v_pk_fma_f16
    }
}

// One position for the pairs of thread j: FIRST = first position of a pass (no predecessor cost; pre >= 0 restricts the predecessor).
// Returns the thread's back-pointer word for this position.
template <int K, int CB, bool FIRST>
__device__ __forceinline__ uint32_t qt_step(int j, half2_t w2, const half_t* __restrict__ c_prev, uint32_t* __restrict__ c_cur, int pre)
{
    constexpr int Kr = 16 - K, NT = qt_nt(K), NI = qt_ni(K), PSH = 16 - 2 * K;
    constexpr uint32_t M = qt_mult<CB>(), STEP = M << Kr, KMASK = (1u << K) - 1u;
    // unrolled body: one chunk of KC candidates (the compiler hoists the LDS reads and products of a longer unrolled run out of the
    // 64-register budget); the pair and chunk loops stay loops
    constexpr int KC = (1 << K) < 16 ? (1 << K) : 16;
    uint32_t bits = 0;
    #pragma unroll 1
    for (int i = 0; i < NI; ++i)
    {
        const int p = j + NT * i;
        const int e0 = 2 * p;
        const int base = K == 8 ? 0 : (e0 >> K);
        uint32_t pr0 = cb_product<CB>((uint32_t) e0);
        uint32_t pr1 = pr0 + M;
        uint32_t best0 = 0xffffffffu, best1 = 0xffffffffu;
        #pragma unroll 1
        for (int kc = 0; kc < (1 << K); kc += KC)
        {
            #pragma unroll
            for (int kk = 0; kk < KC; ++kk)
            {
                const int k = kc + kk;
                half2_t dl = qt_decode2<CB>(pr0, pr1) - w2;
                uint32_t cu;
                if constexpr (FIRST)
                {
                    cu = half2_as_u32(dl * dl);
                    if (pre >= 0 && ((k << PSH) | base) != pre) cu = 0x7c007c00u;
                }
                else
                {
                    half_t cp = c_prev[base + (k << PSH)];
                    half2_t cp2 = { cp, cp };
                    cu = half2_as_u32(__builtin_elementwise_fma(dl, dl, cp2));
                }
                best0 = min(best0, (cu << 16) | (uint32_t) k);
                best1 = min(best1, (cu & 0xffff0000u) | (uint32_t) k);
                pr0 += STEP;
                pr1 += STEP;
            }
        }
        c_cur[p] = (best0 >> 16) | (best1 & 0xffff0000u);
        bits |= ((best0 & KMASK) | ((best1 & KMASK) << K)) << (i * 2 * K);
    }
    return bits;
}

// winning k of node e at position t, from the workspace words of one tile
template <int K>
__device__ __forceinline__ int qt_pred(const uint8_t* __restrict__ ws, int t, int e)
{
    constexpr int NT = qt_nt(K), WB = qt_word_bytes(K), PSH = 16 - 2 * K;
    const int p = e >> 1, j = p % NT, i = p / NT;
    uint32_t word = WB == 4 ? ((const uint32_t*) ws)[t * NT + j] : (uint32_t) ((const uint16_t*) ws)[t * NT + j];
    uint32_t k = (word >> ((2 * i + (e & 1)) * K)) & ((1u << K) - 1u);
    return (int) ((k << PSH) | (uint32_t) (e >> K));
}

// argmin order of the reference's 1024-thread, two-level shuffle-down reduction (quantize_tiles_kernel.cuh:219-268): for v = e mod 1024 the
// virtual thread slot is s = 16 (v >> 9) + ((v >> 5) & 15), lane l = v & 31; leaf order of a shuffle-down tree is bit-reversed, so ties go to the
// smallest (bitrev5(s), bitrev5(l), e >> 10).  rank is that 15-bit key; qt_unrank inverts it.
__device__ __forceinline__ uint32_t qt_brev5(uint32_t x) { return __builtin_bitreverse32(x) >> 27; }
__device__ __forceinline__ uint32_t qt_rank(uint32_t e)
{
    uint32_t v = e & 1023u, s = 16u * (v >> 9) + ((v >> 5) & 15u), l = v & 31u;
    return (qt_brev5(s) << 10) | (qt_brev5(l) << 5) | (e >> 10);
}
__device__ __forceinline__ uint32_t qt_unrank(uint32_t r)
{
    uint32_t s = qt_brev5(r >> 10), l = qt_brev5((r >> 5) & 31u);
    return ((r & 31u) << 10) | ((s >> 4) << 9) | ((s & 15u) << 5) | l;
}

template <int K, int CB>
__global__ __launch_bounds__(qt_nt(K)) __attribute__((amdgpu_waves_per_eu(qt_waves_per_simd(K), qt_waves_per_simd(K))))
void exl3_quantize_tiles_kernel(const float* __restrict__ input, float* __restrict__ output, uint16_t* __restrict__ indices,
                                uint8_t* __restrict__ workspace)
{
    constexpr int E = 65536 >> K, NT = qt_nt(K), NW = NT / 64, WB = qt_word_bytes(K);
    __shared__ uint32_t s_cost[2][E / 2];
    __shared__ half_t s_w[256];
    __shared__ uint16_t s_idx[256];
    __shared__ uint32_t s_red[NW];
    __shared__ int s_pre;

    const int j = threadIdx.x;
    const int64_t tile = blockIdx.x;
    uint8_t* ws = workspace + tile * (int64_t) (256 * NT * WB);
    for (int t = j; t < 256; t += NT) s_w[t] = (half_t) input[tile * 256 + t];
    __syncthreads();

    int pre = -1;
    for (int pass = 0; pass < 2; ++pass)
    {
        // pass 0 visits positions 128..255, 0..127 unconstrained; pass 1 visits 0..255 with the predecessor of position 0 fixed to `pre`
        const int roll = pass == 0 ? 128 : 0;
        int cur = 0;
        for (int step = 0; step < 256; ++step)
        {
            const int t = (step + roll) & 255;
            const half_t w = s_w[t];
            const half2_t w2 = { w, w };
            uint32_t bits = step == 0 ? qt_step<K, CB, true>(j, w2, nullptr, s_cost[cur], pre)
                                      : qt_step<K, CB, false>(j, w2, (const half_t*) s_cost[cur ^ 1], s_cost[cur], pre);
            if constexpr (WB == 4) ((uint32_t*) ws)[t * NT + j] = bits;
            else ((uint16_t*) ws)[t * NT + j] = (uint16_t) bits;
            __syncthreads();
            cur ^= 1;
        }
        const half_t* c_fin = (const half_t*) s_cost[cur ^ 1];

        if (pass == 0)
        {
            uint32_t best = 0xffffffffu;
            for (int e = j; e < E; e += NT)
                best = min(best, ((uint32_t) half_as_u16(c_fin[e]) << 16) | qt_rank((uint32_t) e));
            #pragma unroll
            for (int o = 32; o > 0; o >>= 1) best = min(best, (uint32_t) __shfl_xor((int) best, o));
            if ((j & 63) == 0) s_red[j >> 6] = best;
            __syncthreads();
            if (j == 0)
            {
                for (int w_ = 1; w_ < NW; ++w_) best = min(best, s_red[w_]);
                // trace back from the cheapest end node through positions 127 .. 0: the node reached precedes position 0
                int e = (int) qt_unrank(best & 0xffffu);
                for (int t = 127; t >= 0; --t) e = qt_pred<K>(ws, t, e);
                s_pre = e;
            }
            __syncthreads();
            pre = s_pre;
        }
    }

    // tail-biting trace back from node `pre` at position 255, no argmin
    if (j == 0)
    {
        int e = pre;
        for (int t = 255; t >= 0; --t)
        {
            int p = qt_pred<K>(ws, t, e);
            s_idx[t] = (uint16_t) ((p << K) | e);
            e = p;
        }
    }
    __syncthreads();
    for (int t = j; t < 256; t += NT)
    {
        uint16_t s = s_idx[t];
        indices[tile * 256 + t] = s;
        output[tile * 256 + t] = (float) decode_exact<CB>((uint32_t) s);
    }
}

}  // namespace

#define QT_CAT2(a, b) a##b
#define QT_CAT(a, b) QT_CAT2(a, b)

// per-K launcher (called from exl3_quantize.hip): tiles [0, num_tiles) in launches of at most max_batch tiles, workspace = max_batch tiles
void QT_CAT(exl3_quantize_tiles_launch_k, G2_K)(const float* input, float* output, uint16_t* indices, uint8_t* workspace, int64_t num_tiles,
                                                int64_t max_batch, int cb, hipStream_t stream)
{
    for (int64_t b0 = 0; b0 < num_tiles; b0 += max_batch)
    {
        const int64_t n = num_tiles - b0 < max_batch ? num_tiles - b0 : max_batch;
        const float* in = input + b0 * 256;
        float* out = output + b0 * 256;
        uint16_t* idx = indices + b0 * 256;
        #define QT_L(CC) exl3_quantize_tiles_kernel<G2_K, CC><<<dim3((unsigned) n), dim3(qt_nt(G2_K)), 0, stream>>>(in, out, idx, workspace)
        if (cb == EXL3_CB_3INST) QT_L(EXL3_CB_3INST);
        else if (cb == EXL3_CB_MCG) QT_L(EXL3_CB_MCG);
        else QT_L(EXL3_CB_MUL1);
        #undef QT_L
    }
}

int64_t QT_CAT(exl3_quantize_tiles_ws_bytes_k, G2_K)() { return (int64_t) 256 * qt_nt(G2_K) * qt_word_bytes(G2_K); }
