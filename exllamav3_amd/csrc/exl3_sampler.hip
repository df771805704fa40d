// Device-side token generation: logits -> token (exl3_sample) and token -> next input row (exl3_gen_feed).  gfx950 only.
//
// Semantics: the modes of the reference's fused sampler (exllamav3_ext/generator/sampling_fused.cu:11-30 greedy / Gumbel / Gumbel over the min-p set,
// :156-173 top-k / top-p / min-p as ONE cutoff of the same ordering; sampling_basic.cu: argmax with the lowest index among equals; gumbel.cu: a sample of
// softmax(l / T) is argmax(l / T + g), g ~ Gumbel(0, 1)), restated so that they are exact on fp16 logits (include/exl3_hip.h).  The noise is this project's own
// stream -- Philox4x32-10 keyed (seed) and counted (index, row, step) -- not curand's sequence.
//
// Two kernels, no workgroup ever waits for another:
//   smp_select_kernel  (modes 2, 3) one 16-wave workgroup per row, the 250 KB row re-read from L2 per pass: row maximum, then the cutoff.  fp16 has 65 536
//                      values, so the k-th largest logit is found EXACTLY by a two-level radix select over the order-preserving 16-bit key (256 + 256 integer
//                      bins in LDS); top-p walks the same two levels with masses in 2^40 fixed point (u64 integer adds: independent of arrival order).
//   smp_pick_kernel    (all modes) up to 64 workgroups per row, each the arg-max of its column range of  key  (mode 0) or  l * inv_temp + g  (modes 1-3, over
//                      l >= cutoff); partial results go to the workspace and the LAST workgroup to arrive (atomic ticket, as the split-k finish of the GEMV does)
//                      combines them alone.  Ties go to the lowest index in every mode: the winner is the maximum of (score, ~index).
// Launches per sampled token: mode 0 / 1: one; mode 2 / 3: two; + one for exl3_gen_feed.
#include "exl3_api_internal.h"
#include "exl3_common.cuh"
#include <math.h>

#define SMP_MAX_ROWS     16
#define SMP_MAX_SPLIT    64                 // workgroups per row of the pick kernel (one wave combines them)
#define SMP_COLS_PER_WG  2048
#define SMP_ROW_WS_U64   512                // workspace per row: 4 KiB = [0] cutoff (float bits) [1] ticket [8 + 4 g ...] partial of workgroup g
// keys: -Inf 0x03ff; finite values 0x0400 .. 0xfbff; +Inf 0xfc00; NaN above that or below 0x03ff

// order-preserving 16-bit key of an fp16 bit pattern (-0 counts as +0: they are equal as values)
__device__ __forceinline__ uint32_t smp_key(uint32_t u)
{
    u = u == 0x8000u ? 0u : u;
    return u ^ ((u & 0x8000u) ? 0xffffu : 0x8000u);
}
// on the raw bits: finite = exponent not all ones (what is left is NaN, +Inf -- an invalid row -- or -Inf = 0xfc00, never chosen)
__device__ __forceinline__ bool smp_finite_bits(uint32_t u) { return (u & 0x7c00u) != 0x7c00u; }
__device__ __forceinline__ float smp_key_value(uint32_t key)
{
    const uint32_t u = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
    return (float) u16_as_half(u);
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), output word 0
__device__ __forceinline__ uint32_t smp_philox_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    #pragma unroll
    for (int r = 0; r < 10; ++r)
    {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
// u = ((w >> 9) + 0.5) * 2^-23: exact in fp32, strictly inside (0, 1);  g = -log(-log(u))
__device__ __forceinline__ float smp_gumbel(uint32_t w)
{
    const float u = ((float) (w >> 9) + 0.5f) * 1.1920928955078125e-07f;
    return -logf(-logf(u));
}
__device__ __forceinline__ uint32_t smp_float_key(float v)
{
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ unsigned long long smp_wave_max_u64(unsigned long long v)
{
    #pragma unroll
    for (int i = 1; i < 64; i <<= 1)
    {
        const unsigned long long o = ((unsigned long long) xor_lane_u32((uint32_t) (v >> 32), i) << 32) | xor_lane_u32((uint32_t) v, i);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t smp_wave_max(uint32_t v)
{
    #pragma unroll
    for (int i = 1; i < 64; i <<= 1) { const uint32_t o = xor_lane_u32(v, i); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t smp_wave_min(uint32_t v)
{
    #pragma unroll
    for (int i = 1; i < 64; i <<= 1) { const uint32_t o = xor_lane_u32(v, i); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t smp_wave_sum(uint32_t v)
{
    #pragma unroll
    for (int i = 1; i < 64; i <<= 1) v += xor_lane_u32(v, i);
    return v;
}
__device__ __forceinline__ uint32_t smp_wave_or(uint32_t v)
{
    #pragma unroll
    for (int i = 1; i < 64; i <<= 1) v |= xor_lane_u32(v, i);
    return v;
}

// f(index, fp16 bits) for every column in [begin, end) below `size`: 16-byte loads (begin and ld are multiples of 8, so a load never leaves the row), four of
// them in flight per thread -- a lone workgroup walking a 250 KB row is bound by the latency of its loads, not by their number
template <typename F>
__device__ __forceinline__ void smp_for_each(const half_t* __restrict__ row, int begin, int end, int size, int tid, int nthreads, F f)
{
    const int stride = 8 * nthreads, lim = end < size ? end : size;
    auto eight = [&] (int c, const uint4_t v)
    {
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
        if (c + 8 <= lim)
        {
            #pragma unroll
            for (int j = 0; j < 8; ++j) f(c + j, (w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
        }
        else
        {
            #pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c + j < lim) f(c + j, (w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
        }
    };
    int c = begin + 8 * tid;
    for (; c + 3 * stride < end; c += 4 * stride)
    {
        const uint4_t v0 = *(const uint4_t*) (row + c), v1 = *(const uint4_t*) (row + c + stride), v2 = *(const uint4_t*) (row + c + 2 * stride),
                      v3 = *(const uint4_t*) (row + c + 3 * stride);
        eight(c, v0); eight(c + stride, v1); eight(c + 2 * stride, v2); eight(c + 3 * stride, v3);
    }
    for (; c < end; c += stride) eight(c, *(const uint4_t*) (row + c));
}

// S[t] = sum of v over bins >= t, t = 0 .. 255 (threads 0 .. 255 pass their bin's value), S[256] = 0.  Whole workgroup calls it.
__device__ __forceinline__ void smp_suffix256(unsigned long long v, unsigned long long* __restrict__ S, unsigned long long* __restrict__ wtot, int tid)
{
    if (tid < 256)
    {
        const int lane = tid & 63;
        #pragma unroll
        for (int o = 1; o < 64; o <<= 1)
        {
            const unsigned long long n = __shfl_down(v, o, 64);
            if (lane + o < 64) v += n;
        }
        if (lane == 0) wtot[tid >> 6] = v;
    }
    __syncthreads();
    if (tid < 256)
    {
        for (int w = (tid >> 6) + 1; w < 4; ++w) v += wtot[w];
        S[tid] = v;
    }
    if (tid == 256) S[256] = 0;
    __syncthreads();
}

// ---- cutoff of modes 2 / 3: one workgroup per row ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024)
void smp_select_kernel(const half_t* __restrict__ logits, int ld, int size, int mode, int filters, int top_k, float top_p, float inv_temp_filter, float minp_log,
                       unsigned long long* __restrict__ ws)
{
    __shared__ uint32_t cnt[8 * 256];                 // 8 copies (lane & 7) of a 256-bin histogram: fewer same-address collisions inside a wave
    __shared__ unsigned long long mass[8 * 256];
    __shared__ unsigned long long S[257];
    __shared__ unsigned long long wtot[4];
    __shared__ uint32_t red[32];
    __shared__ int sel_bin;
    __shared__ unsigned long long sel_above;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x, cp = (tid & 7) * 256;
    const half_t* rp = logits + (size_t) row * ld;
    float* cutoff_w = (float*) (ws + (size_t) row * SMP_ROW_WS_U64);
    const bool do_k = mode == 3 && (filters & 1), do_p = mode == 3 && (filters & 2), do_m = mode == 2 || (mode == 3 && (filters & 4));

    for (int i = tid; i < 8 * 256; i += 1024) { cnt[i] = 0; mass[i] = 0; }
    if (tid == 0) sel_bin = -1;
    __syncthreads();
    // pass 1: validity, row maximum, counts by the key's high byte
    uint32_t kmax = 0, flags = 0;
    smp_for_each(rp, 0, size, size, tid, 1024, [&] (int, uint32_t u)
    {
        if (!smp_finite_bits(u)) { if (u != 0xfc00u) flags |= 1; return; }
        const uint32_t key = smp_key(u);
        flags |= 2;
        kmax = key > kmax ? key : kmax;
        if (do_k) atomicAdd(&cnt[cp + (key >> 8)], 1u);
    });
    kmax = smp_wave_max(kmax); flags = smp_wave_or(flags);
    if (lane == 0) { red[wave] = kmax; red[16 + wave] = flags; }
    __syncthreads();
    kmax = 0; flags = 0;
    for (int w = 0; w < 16; ++w) { kmax = red[w] > kmax ? red[w] : kmax; flags |= red[16 + w]; }
    if ((flags & 1) || !(flags & 2))
    {
        if (tid == 0) *cutoff_w = INFINITY;               // invalid row: the pick kernel sees the same flags and answers -1
        return;
    }
    const float M = smp_key_value(kmax);
    float c0 = -INFINITY;
    if (do_k)
    {
        const unsigned long long k = (unsigned long long) top_k;
        unsigned long long v = 0;
        if (tid < 256) for (int c = 0; c < 8; ++c) v += cnt[c * 256 + tid];
        smp_suffix256(v, S, wtot, tid);
        if (tid < 256 && S[tid] >= k && S[tid + 1] < k) { sel_bin = tid; sel_above = S[tid + 1]; }
        __syncthreads();
        const int b1 = sel_bin;
        const unsigned long long above = sel_above;
        uint32_t ck = 0x0400u;                             // fewer than k finite values: all of them
        if (b1 >= 0)
        {
            for (int i = tid; i < 8 * 256; i += 1024) cnt[i] = 0;
            __syncthreads();
            if (tid == 0) sel_bin = -1;
            smp_for_each(rp, 0, size, size, tid, 1024, [&] (int, uint32_t u)
            {
                const uint32_t key = smp_key(u);
                if (smp_finite_bits(u) && (int) (key >> 8) == b1) atomicAdd(&cnt[cp + (key & 255u)], 1u);
            });
            __syncthreads();
            v = 0;
            if (tid < 256) for (int c = 0; c < 8; ++c) v += cnt[c * 256 + tid];
            smp_suffix256(v, S, wtot, tid);
            if (tid < 256 && above + S[tid] >= k && above + S[tid + 1] < k) sel_bin = tid;
            __syncthreads();
            ck = ((uint32_t) b1 << 8) | (uint32_t) sel_bin;
        }
        c0 = smp_key_value(ck);
        __syncthreads();
    }
    if (do_m)
    {
        const float thr = M + minp_log;                    // one fp32 add
        c0 = thr > c0 ? thr : c0;
    }
    float cutoff = c0;
    if (do_p)
    {
        if (tid == 0) sel_bin = -1;
        __syncthreads();
        // pass 3: 2^40 fixed-point masses of the survivors by the key's high byte
        smp_for_each(rp, 0, size, size, tid, 1024, [&] (int, uint32_t u)
        {
            const float l = (float) u16_as_half(u);
            if (smp_finite_bits(u) && l >= c0)
                atomicAdd(&mass[cp + (smp_key(u) >> 8)], (unsigned long long) (expf((l - M) * inv_temp_filter) * 1099511627776.0f));
        });
        __syncthreads();
        unsigned long long v = 0;
        if (tid < 256) for (int c = 0; c < 8; ++c) v += mass[c * 256 + tid];
        smp_suffix256(v, S, wtot, tid);
        const unsigned long long T = (unsigned long long) __double2ull_rd((double) top_p * (double) S[0]);
        if (tid < 256 && S[tid] > T && S[tid + 1] <= T) { sel_bin = tid; sel_above = S[tid + 1]; }
        __syncthreads();
        const int B = sel_bin;
        const unsigned long long above = sel_above;
        if (B >= 0)                                        // (B < 0: the whole surviving mass is within p * Z -- nothing to cut)
        {
            for (int i = tid; i < 8 * 256; i += 1024) mass[i] = 0;
            __syncthreads();
            if (tid == 0) sel_bin = 256;
            smp_for_each(rp, 0, size, size, tid, 1024, [&] (int, uint32_t u)
            {
                const uint32_t key = smp_key(u);
                const float l = (float) u16_as_half(u);
                if (smp_finite_bits(u) && l >= c0 && (int) (key >> 8) == B)
                    atomicAdd(&mass[cp + (key & 255u)], (unsigned long long) (expf((l - M) * inv_temp_filter) * 1099511627776.0f));
            });
            __syncthreads();
            v = 0;
            if (tid < 256) for (int c = 0; c < 8; ++c) v += mass[c * 256 + tid];
            smp_suffix256(v, S, wtot, tid);
            // the value classes of bin B that stay: above + S[t] <= T holds from some t0 upwards (t0 = 256: none of them)
            if (tid < 256 && above + S[tid] <= T && (tid == 0 || above + S[tid - 1] > T)) sel_bin = tid;
            __syncthreads();
            uint32_t pk = ((uint32_t) B << 8) + (uint32_t) sel_bin;
            pk = pk > kmax ? kmax : pk;                    // the top class always stays
            const float cpv = smp_key_value(pk);
            cutoff = cpv > cutoff ? cpv : cutoff;
        }
    }
    if (tid == 0) *cutoff_w = cutoff;
}

// ---- the token: arg-max over column ranges, combined by the last workgroup to arrive ------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void smp_pick_kernel(const half_t* __restrict__ logits, int ld, int size, int chunk, int mode, float inv_temp, uint32_t seed_lo, uint32_t seed_hi,
                     const long long* __restrict__ step_ptr, int row0, unsigned long long* __restrict__ ws, int32_t* __restrict__ tokens,
                     float* __restrict__ cutoff_out, int32_t* __restrict__ kept_out)
{
    __shared__ unsigned long long best_s[4];
    __shared__ uint32_t red[12];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.y, g = blockIdx.x, G = gridDim.x;
    const half_t* rp = logits + (size_t) row * ld;
    unsigned long long* wr = ws + (size_t) row * SMP_ROW_WS_U64;
    const float cutoff = mode >= 2 ? *(const float*) wr : -INFINITY;
    const unsigned long long step = step_ptr ? (unsigned long long) *step_ptr : 0ull;
    const uint32_t c1 = (uint32_t) (row0 + row), c2 = (uint32_t) step, c3 = (uint32_t) (step >> 32);

    unsigned long long best = 0;
    uint32_t kept = 0, minkey = 0xffffu, flags = 0;
    const int begin = g * chunk, end = min(begin + chunk, size);
    smp_for_each(rp, begin, end, size, tid, 256, [&] (int idx, uint32_t u)
    {
        if (!smp_finite_bits(u)) { if (u != 0xfc00u) flags |= 1; return; }
        const uint32_t key = smp_key(u);
        flags |= 2;
        const float l = (float) u16_as_half(u);
        if (mode >= 2 && !(l >= cutoff)) return;
        kept += 1;
        minkey = key < minkey ? key : minkey;
        uint32_t score = key;
        if (mode != 0)
        {
            float v = l * inv_temp;
            v = v + smp_gumbel(smp_philox_w0((uint32_t) idx, c1, c2, c3, seed_lo, seed_hi));
            v = v + 0.0f;                                  // (-0 -> +0: equal values, equal scores)
            score = smp_float_key(v);
        }
        const unsigned long long cand = ((unsigned long long) score << 32) | (0xffffffffu - (uint32_t) idx);
        best = cand > best ? cand : best;
    });
    best = smp_wave_max_u64(best); kept = smp_wave_sum(kept); minkey = smp_wave_min(minkey); flags = smp_wave_or(flags);
    if (lane == 0) { best_s[wave] = best; red[wave] = kept; red[4 + wave] = minkey; red[8 + wave] = flags; }
    __syncthreads();
    if (tid == 0)
    {
        for (int w = 1; w < 4; ++w)
        {
            best = best_s[w] > best ? best_s[w] : best; kept += red[w]; minkey = red[4 + w] < minkey ? red[4 + w] : minkey; flags |= red[8 + w];
        }
        unsigned long long* p = wr + 8 + 4 * g;
        __hip_atomic_store(p, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p + 1, ((unsigned long long) minkey << 32) | kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p + 2, (unsigned long long) flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const uint32_t old = atomicAdd((uint32_t*) (wr + 1), 1u);
        last_s = old == (uint32_t) (G - 1);
    }
    __syncthreads();
    if (!last_s || wave != 0) return;
    // the last workgroup to arrive: every partial of this row is visible (release by its writer before the ticket, acquire here)
    __threadfence();
    best = 0; kept = 0; minkey = 0xffffu; flags = 0;
    if (lane < G)
    {
        unsigned long long* p = wr + 8 + 4 * lane;
        best = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long km = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        kept = (uint32_t) km; minkey = (uint32_t) (km >> 32);
        flags = (uint32_t) __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    best = smp_wave_max_u64(best); kept = smp_wave_sum(kept); minkey = smp_wave_min(minkey); flags = smp_wave_or(flags);
    if (lane == 0)
    {
        const bool ok = !(flags & 1) && (flags & 2) && kept > 0;
        tokens[row] = ok ? (int32_t) (0xffffffffu - (uint32_t) best) : -1;
        if (cutoff_out) cutoff_out[row] = ok ? smp_key_value(minkey) : NAN;      // the smallest kept logit
        if (kept_out) kept_out[row] = ok ? (int32_t) kept : 0;
        __hip_atomic_store((uint32_t*) (wr + 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the ticket is left zeroed
    }
}

// ---- token -> next input row -------------------------------------------------------------------------------------------------------------------------------
// One workgroup for all rows (m <= 16): every thread reads the step word before the barrier, thread 0 advances it after.
__global__ __launch_bounds__(1024)
void gen_feed_kernel(const int32_t* __restrict__ sampled, const int32_t* __restrict__ forced, int forced_len, int m, const half_t* __restrict__ embed, int vocab,
                     int hidden, half_t* __restrict__ x0, int32_t* __restrict__ tokens_out, int out_len, int32_t* __restrict__ positions,
                     int32_t* __restrict__ cache_seqlens, int32_t* __restrict__ attn_lens, int32_t* __restrict__ invalid, long long* __restrict__ step_ptr)
{
    __shared__ int tok_s[SMP_MAX_ROWS];
    const int tid = threadIdx.x;
    const long long step = *step_ptr;
    if (tid < m)
    {
        int tok = -1;
        if (forced && step + 1 >= 0 && step + 1 < forced_len) tok = forced[(size_t) tid * forced_len + (step + 1)];
        else if (sampled) tok = sampled[tid];
        if (tok < 0 || tok >= vocab || invalid[tid]) { tok = -1; invalid[tid] = 1; }        // sticky: never indexes the table
        tok_s[tid] = tok;
        if (tokens_out && step >= 0 && step < out_len) tokens_out[(size_t) tid * out_len + step] = tok;
        if (positions) positions[tid] += 1;
        if (cache_seqlens) cache_seqlens[tid] += 1;
        if (attn_lens) attn_lens[tid] += 1;
    }
    __syncthreads();
    const int per_row = hidden / 8;
    for (int i = tid; i < m * per_row; i += 1024)
    {
        const int r = i / per_row, c = i - r * per_row, tok = tok_s[r];
        if (tok >= 0) ((uint4_t*) (x0 + (size_t) r * hidden))[c] = ((const uint4_t*) (embed + (size_t) tok * hidden))[c];
    }
    if (tid == 0) *step_ptr = step + 1;
}

// exl3_gen_feed with stop tokens: a row whose SAMPLED token is one of stop_ids becomes done (sticky).  The stop token is recorded but not fed: from that step on
// the row's input, positions and lengths stay as they are (the step keeps rewriting one cache slot) and tokens_out receives pad_token.  live = rows neither done
// nor invalid behind this step.
#define GEN_MAX_STOP 64
__global__ __launch_bounds__(1024)
void gen_feed_stop_kernel(const int32_t* __restrict__ sampled, const int32_t* __restrict__ forced, int forced_len, int m, const half_t* __restrict__ embed, int vocab,
                          int hidden, half_t* __restrict__ x0, int32_t* __restrict__ tokens_out, int out_len, int32_t* __restrict__ positions,
                          int32_t* __restrict__ cache_seqlens, int32_t* __restrict__ attn_lens, int32_t* __restrict__ invalid, long long* __restrict__ step_ptr,
                          const int32_t* __restrict__ stop_ids, int n_stop, int32_t* __restrict__ done, int pad_token, int32_t* __restrict__ live)
{
    __shared__ int tok_s[SMP_MAX_ROWS];
    __shared__ int live_s[SMP_MAX_ROWS];
    const int tid = threadIdx.x;
    const long long step = *step_ptr;
    if (tid < m)
    {
        int tok = -1, feed = -1;
        if (done[tid]) tok = pad_token;
        else
        {
            bool is_sampled = false;
            if (forced && step + 1 >= 0 && step + 1 < forced_len) tok = forced[(size_t) tid * forced_len + (step + 1)];
            else if (sampled) { tok = sampled[tid]; is_sampled = true; }
            if (tok < 0 || tok >= vocab || invalid[tid]) { tok = -1; invalid[tid] = 1; }        // sticky: never indexes the table
            bool stop = false;
            if (is_sampled && tok >= 0)
                for (int k = 0; k < n_stop; ++k) stop = stop || stop_ids[k] == tok;
            if (stop) done[tid] = 1;
            else
            {
                feed = tok;
                if (positions) positions[tid] += 1;
                if (cache_seqlens) cache_seqlens[tid] += 1;
                if (attn_lens) attn_lens[tid] += 1;
            }
        }
        tok_s[tid] = feed;
        live_s[tid] = !done[tid] && !invalid[tid];
        if (tokens_out && step >= 0 && step < out_len) tokens_out[(size_t) tid * out_len + step] = tok;
    }
    __syncthreads();
    const int per_row = hidden / 8;
    for (int i = tid; i < m * per_row; i += 1024)
    {
        const int r = i / per_row, c = i - r * per_row, tok = tok_s[r];
        if (tok >= 0) ((uint4_t*) (x0 + (size_t) r * hidden))[c] = ((const uint4_t*) (embed + (size_t) tok * hidden))[c];
    }
    if (tid == 0)
    {
        int n = 0;
        for (int r = 0; r < m; ++r) n += live_s[r];
        *live = n;
        *step_ptr = step + 1;
    }
}

// ---- prompt ids -> input rows of a prefill chunk --------------------------------------------------------------------------------------------------------------
// out[b * T + t] = embed[ids[b][col0 + t]]: one workgroup per output row, 16-byte copies.  The feed's rules for a bad id: it never indexes the table, the row is
// written as zeros and invalid[b] is set (only ever set here, so rows of one sequence may race on it).
__global__ __launch_bounds__(256)
void embed_rows_kernel(const int32_t* __restrict__ ids, int ld_ids, int col0, int T, const half_t* __restrict__ embed, int vocab, int hidden,
                       half_t* __restrict__ out, int32_t* __restrict__ invalid)
{
    const int row = blockIdx.x, b = row / T, t = row - b * T;
    const int tok = ids[(size_t) b * ld_ids + col0 + t];
    const bool ok = tok >= 0 && tok < vocab;
    if (!ok && threadIdx.x == 0) invalid[b] = 1;
    const uint4_t* src = (const uint4_t*) (embed + (size_t) (ok ? tok : 0) * hidden);
    uint4_t* dst = (uint4_t*) (out + (size_t) row * hidden);
    const uint4_t zero = {0u, 0u, 0u, 0u};
    for (int c = threadIdx.x; c < hidden / 8; c += 256) dst[c] = ok ? src[c] : zero;
}

extern "C" int exl3_sample_workspace(int m, int64_t* bytes)
{
    EXL3_CHECK_ARG(m >= 1 && m <= SMP_MAX_ROWS && bytes, "exl3_sample_workspace: m must be in [1, 16]");
    *bytes = (int64_t) m * SMP_ROW_WS_U64 * 8;
    return EXL3_OK;
}

extern "C" int exl3_sample(const void* logits, int m, int ld, int size, int mode, int filters, int top_k, float top_p, float inv_temp, float inv_temp_filter,
                           float minp_log, uint32_t seed_lo, uint32_t seed_hi, const int64_t* step, int row0, void* workspace, int64_t workspace_bytes,
                           int32_t* tokens, float* cutoff_out, int32_t* kept_out, void* stream)
{
    EXL3_CHECK_ARG(m >= 1 && m <= SMP_MAX_ROWS, "exl3_sample: m must be in [1, 16]");
    EXL3_CHECK_ARG(ld >= 8 && ld % 8 == 0 && size >= 1 && size <= ld, "exl3_sample: ld must be a multiple of 8 and 1 <= size <= ld");
    EXL3_CHECK_ARG(mode >= 0 && mode <= 3, "exl3_sample: mode must be in [0, 3]");
    EXL3_CHECK_ARG(logits && tokens && workspace, "exl3_sample: null pointer");
    EXL3_CHECK_ARG(((uintptr_t) logits & 15) == 0, "exl3_sample: logits must be 16-byte aligned");
    EXL3_CHECK_ARG(((uintptr_t) workspace & 7) == 0 && workspace_bytes >= (int64_t) m * SMP_ROW_WS_U64 * 8, "exl3_sample: workspace too small (exl3_sample_workspace)");
    EXL3_CHECK_ARG(row0 >= 0, "exl3_sample: row0 must not be negative");
    if (mode >= 1) EXL3_CHECK_ARG(inv_temp > 0.0f && isfinite(inv_temp), "exl3_sample: inv_temp must be positive and finite");
    if (mode == 3)
    {
        EXL3_CHECK_ARG(filters >= 1 && filters <= 7, "exl3_sample: mode 3 needs filter bits (1 top-k, 2 top-p, 4 min-p)");
        EXL3_CHECK_ARG(!(filters & 1) || top_k >= 1, "exl3_sample: top_k must be at least 1");
        EXL3_CHECK_ARG(!(filters & 2) || (top_p > 0.0f && top_p <= 1.0f && inv_temp_filter > 0.0f && isfinite(inv_temp_filter)),
                       "exl3_sample: top_p must be in (0, 1] and inv_temp_filter positive");
    }
    if (mode == 2 || (mode == 3 && (filters & 4))) EXL3_CHECK_ARG(minp_log <= 0.0f && !isnan(minp_log), "exl3_sample: minp_log must not be positive");
    if (mode >= 2)
    {
        smp_select_kernel<<<m, 1024, 0, (hipStream_t) stream>>>((const half_t*) logits, ld, size, mode, filters, top_k, top_p, inv_temp_filter, minp_log,
                                                                 (unsigned long long*) workspace);
        if (int rc = exl3_check_launch("sample_select")) return rc;
    }
    int G = (size + SMP_COLS_PER_WG - 1) / SMP_COLS_PER_WG;
    G = G > SMP_MAX_SPLIT ? SMP_MAX_SPLIT : G;
    const int chunk = ((size + G - 1) / G + 7) & ~7;
    smp_pick_kernel<<<dim3(G, m), 256, 0, (hipStream_t) stream>>>((const half_t*) logits, ld, size, chunk, mode, inv_temp, seed_lo, seed_hi, (const long long*) step, row0,
                                                                   (unsigned long long*) workspace, tokens, cutoff_out, kept_out);
    return exl3_check_launch("sample_pick");
}

extern "C" int exl3_gen_feed(const int32_t* sampled, const int32_t* forced, int forced_len, int m, const void* embed, int vocab, int hidden, void* x0,
                             int32_t* tokens_out, int out_len, int32_t* positions, int32_t* cache_seqlens, int32_t* attn_lens, int32_t* invalid, int64_t* step,
                             void* stream)
{
    EXL3_CHECK_ARG(m >= 1 && m <= SMP_MAX_ROWS, "exl3_gen_feed: m must be in [1, 16]");
    EXL3_CHECK_ARG(embed && x0 && invalid && step, "exl3_gen_feed: null pointer");
    EXL3_CHECK_ARG(sampled || forced, "exl3_gen_feed: needs sampled or forced tokens");
    EXL3_CHECK_ARG(vocab >= 1 && hidden >= 8 && hidden % 8 == 0, "exl3_gen_feed: hidden must be a multiple of 8");
    EXL3_CHECK_ARG((((uintptr_t) embed | (uintptr_t) x0) & 15) == 0, "exl3_gen_feed: embed / x0 must be 16-byte aligned");
    EXL3_CHECK_ARG(!forced || forced_len >= 1, "exl3_gen_feed: forced_len must be at least 1");
    EXL3_CHECK_ARG(!tokens_out || out_len >= 1, "exl3_gen_feed: out_len must be at least 1");
    gen_feed_kernel<<<1, 1024, 0, (hipStream_t) stream>>>(sampled, forced, forced ? forced_len : 0, m, (const half_t*) embed, vocab, hidden, (half_t*) x0, tokens_out,
                                                          tokens_out ? out_len : 0, positions, cache_seqlens, attn_lens, invalid, (long long*) step);
    return exl3_check_launch("gen_feed");
}

extern "C" int exl3_gen_feed_stop(const int32_t* sampled, const int32_t* forced, int forced_len, int m, const void* embed, int vocab, int hidden, void* x0,
                                  int32_t* tokens_out, int out_len, int32_t* positions, int32_t* cache_seqlens, int32_t* attn_lens, int32_t* invalid, int64_t* step,
                                  const int32_t* stop_ids, int n_stop, int32_t* done, int pad_token, int32_t* live, void* stream)
{
    EXL3_CHECK_ARG(m >= 1 && m <= SMP_MAX_ROWS, "exl3_gen_feed_stop: m must be in [1, 16]");
    EXL3_CHECK_ARG(embed && x0 && invalid && step && done && live, "exl3_gen_feed_stop: null pointer");
    EXL3_CHECK_ARG(sampled || forced, "exl3_gen_feed_stop: needs sampled or forced tokens");
    EXL3_CHECK_ARG(vocab >= 1 && hidden >= 8 && hidden % 8 == 0, "exl3_gen_feed_stop: hidden must be a multiple of 8");
    EXL3_CHECK_ARG((((uintptr_t) embed | (uintptr_t) x0) & 15) == 0, "exl3_gen_feed_stop: embed / x0 must be 16-byte aligned");
    EXL3_CHECK_ARG(!forced || forced_len >= 1, "exl3_gen_feed_stop: forced_len must be at least 1");
    EXL3_CHECK_ARG(!tokens_out || out_len >= 1, "exl3_gen_feed_stop: out_len must be at least 1");
    EXL3_CHECK_ARG(n_stop >= 0 && n_stop <= GEN_MAX_STOP && (n_stop == 0 || stop_ids), "exl3_gen_feed_stop: at most 64 stop ids");
    gen_feed_stop_kernel<<<1, 1024, 0, (hipStream_t) stream>>>(sampled, forced, forced ? forced_len : 0, m, (const half_t*) embed, vocab, hidden, (half_t*) x0, tokens_out,
                                                               tokens_out ? out_len : 0, positions, cache_seqlens, attn_lens, invalid, (long long*) step, stop_ids, n_stop,
                                                               done, pad_token, live);
    return exl3_check_launch("gen_feed_stop");
}

extern "C" int exl3_embed_rows(const int32_t* ids, int ld_ids, int col0, int T, int m, const void* embed, int vocab, int hidden, void* out, int32_t* invalid,
                               void* stream)
{
    EXL3_CHECK_ARG(m >= 1 && m <= SMP_MAX_ROWS, "exl3_embed_rows: m must be in [1, 16]");
    EXL3_CHECK_ARG(ids && embed && out && invalid, "exl3_embed_rows: null pointer");
    EXL3_CHECK_ARG(T >= 1, "exl3_embed_rows: T must be at least 1");
    EXL3_CHECK_ARG(col0 >= 0 && (int64_t) col0 + T <= ld_ids, "exl3_embed_rows: columns [col0, col0 + T) must lie inside the id matrix");
    EXL3_CHECK_ARG(vocab >= 1 && hidden >= 8 && hidden % 8 == 0, "exl3_embed_rows: hidden must be a multiple of 8");
    EXL3_CHECK_ARG((((uintptr_t) embed | (uintptr_t) out) & 15) == 0, "exl3_embed_rows: embed / out must be 16-byte aligned");
    EXL3_CHECK_ARG((int64_t) m * T <= 0x7fffffff, "exl3_embed_rows: too many rows");
    embed_rows_kernel<<<m * T, 256, 0, (hipStream_t) stream>>>(ids, ld_ids, col0, T, (const half_t*) embed, vocab, hidden, (half_t*) out, invalid);
    return exl3_check_launch("embed_rows");
}
