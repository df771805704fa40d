// Logit processors of the device-side generation loop: raw logits -> the row the sampler reads, one launch for up to 16 rows.  gfx950 only.
//
// Semantics: the reference's repetition penalty and presence / frequency penalty (exllamav3_ext/generator/rep_pen.cu: apply_rep_pens, apply_pres_freq_pens; the
// window rule of :51 / :168, the blend of :85-88, the subtraction of :197-198), its dense logit bias (generator/sampler/custom.py:581-609) and its packed token
// bitmask (generator/sampling_fused.cu:951-1020 apply_logit_bitmask), applied in that order in fp32 and rounded once to the output type (include/exl3_hip.h).
// Unlike the reference's kernels it takes up to 16 rows, reads the history where exl3_gen_feed writes it (two int32 segments per row, the length of the second from
// a DEVICE word) and accumulates the window weights as INTEGERS: weight = num / Dn with num an integer, pmax = max(num) by ds_max_u32, fsum = sum(num) by
// ds_add_u32 -- the result does not depend on the arrival order of the atomics, on the grid or on the batch (the reference's atomicAdd(float) does).
//
// One kernel, grid (vocabulary spans of 2048 columns, rows), 256 threads; no workgroup waits for another, no global atomics:
//   1. (penalties on) zero the span's integer tables in LDS (up to 3 x 8 KiB), scan the window of the row's history (L2-resident, coalesced int32 loads) and
//      record the ids that fall into the span;
//   2. every thread streams 8 columns: one 16-byte load (fp16) or two (fp32), the arithmetic, one or two 16-byte stores.  Columns [size, ld) are written -Inf.
#include "exl3_api_internal.h"
#include "exl3_common.cuh"
#include <math.h>

#define LP_MAX_ROWS   16
#define LP_SPAN       2048
#define LP_THREADS    256
#define LP_MAX_HIST   (1 << 30)             // len_a + ldb: every index of the scan and its stride stay inside an int32

struct lp_args
{
    const void* in; void* out;
    int ld, size;
    const int32_t* past_a; int lda, len_a;
    const int32_t* past_b; int ldb, len_b;
    const long long* len_b_dev; int len_b_bias;
    int rep_on, rep_S, rep_D; float rep_p;
    int pf_on, pf_S, pf_D; float pres_p, freq_p;
    const float* bias;
    const uint32_t* bitmask; int bitmask_row_stride, bitmask_words;
};

__device__ __forceinline__ bool lp_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// weight numerator of a past token at distance dist (1 = newest) under (S, D): 0 = does not count
__device__ __forceinline__ uint32_t lp_num(int dist, int S, int D)
{
    if ((long long) dist >= (long long) S + D) return 0u;
    if (dist <= S) return (uint32_t) (D > 0 ? D : 1);
    return (uint32_t) (D - (dist - S));
}

template <typename TI, typename TO>
__global__ __launch_bounds__(LP_THREADS)
void lp_kernel(const lp_args a)
{
    extern __shared__ uint32_t lp_tab[];
    const int tid = threadIdx.x, row = blockIdx.y, begin = blockIdx.x * LP_SPAN;
    uint32_t* rep_max = lp_tab;
    uint32_t* pf_max = lp_tab + (a.rep_on ? LP_SPAN : 0);
    uint32_t* pf_sum = pf_max + LP_SPAN;

    if (a.rep_on || a.pf_on)
    {
        const int ntab = (a.rep_on ? 1 : 0) + (a.pf_on ? 2 : 0);
        for (int i = tid; i < ntab * LP_SPAN; i += LP_THREADS) lp_tab[i] = 0u;
        __syncthreads();
        long long lb = a.len_b;
        if (a.len_b_dev)
        {
            lb = *a.len_b_dev + (long long) a.len_b_bias;
            lb = lb < 0 ? 0 : (lb > (long long) a.ldb ? (long long) a.ldb : lb);
        }
        const int n = a.len_a + (int) lb;
        const int32_t* pa = a.past_a + (size_t) row * a.lda;
        const int32_t* pb = a.past_b + (size_t) row * a.ldb;
        const long long w_rep = a.rep_on ? (long long) a.rep_S + a.rep_D : 0, w_pf = a.pf_on ? (long long) a.pf_S + a.pf_D : 0;
        const long long w = w_rep > w_pf ? w_rep : w_pf;                     // a token counts iff dist < w: indices n - w + 1 .. n - 1
        const long long first = (long long) n - w + 1;
        const int lim = begin + LP_SPAN < a.size ? begin + LP_SPAN : a.size;
        for (int i = (first > 0 ? (int) first : 0) + tid; i < n; i += LP_THREADS)
        {
            const int t = i < a.len_a ? pa[i] : pb[i - a.len_a];
            if (t < begin || t >= lim) continue;                                // (ids outside [0, size) are ignored with the rest)
            const int dist = n - i;
            if (a.rep_on)
            {
                const uint32_t num = lp_num(dist, a.rep_S, a.rep_D);
                if (num) atomicMax(&rep_max[t - begin], num);
            }
            if (a.pf_on)
            {
                const uint32_t num = lp_num(dist, a.pf_S, a.pf_D);
                if (num) { atomicMax(&pf_max[t - begin], num); atomicAdd(&pf_sum[t - begin], num); }
            }
        }
        __syncthreads();
    }

    const int c = begin + 8 * tid;
    if (c >= a.ld) return;
    float v[8];
    if constexpr (sizeof(TI) == 2)
    {
        const uint4_t q = *(const uint4_t*) ((const half_t*) a.in + (size_t) row * a.ld + c);
        const uint32_t w4[4] = { q.x, q.y, q.z, q.w };
        #pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float) u16_as_half((w4[j >> 1] >> (16 * (j & 1))) & 0xffffu);
    }
    else
    {
        const float4_t* p = (const float4_t*) ((const float*) a.in + (size_t) row * a.ld + c);
        const float4_t q0 = p[0], q1 = p[1];
        v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
    }
    // the 8 columns lie inside one word of the bitmask (c is a multiple of 8)
    uint32_t keep = 0xffu;
    if (a.bitmask)
    {
        const int wi = c >> 5;
        keep = wi < a.bitmask_words ? (a.bitmask[(size_t) row * a.bitmask_row_stride + wi] >> (c & 31)) & 0xffu : 0u;
    }
    float b[8] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (a.bias)
    {
        if (c + 8 <= a.size)                                                    // (c is a multiple of 8: 32-byte aligned in the fp32 vector)
        {
            const float4_t b0 = ((const float4_t*) (a.bias + c))[0], b1 = ((const float4_t*) (a.bias + c))[1];
            b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w; b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
        }
        else
        {
            #pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c + j < a.size) b[j] = a.bias[c + j];
        }
    }
    const float rep_dn = (float) (a.rep_D > 0 ? a.rep_D : 1), pf_dn = (float) (a.pf_D > 0 ? a.pf_D : 1);
    #pragma unroll
    for (int j = 0; j < 8; ++j)
    {
        const int t = c + j;
        float x = v[j];
        if (t >= a.size) { v[j] = -INFINITY; continue; }
        if (a.rep_on)
        {
            const uint32_t pm = rep_max[t - begin];
            if (pm > 0u && lp_finite(x))
            {
                const float w = x > 0.0f ? x / a.rep_p : x * a.rep_p;
                const float f = (float) pm / rep_dn;
                x = (x * (1.0f - f)) + (w * f);
            }
        }
        if (a.pf_on)
        {
            const uint32_t pm = pf_max[t - begin];
            if (pm > 0u && lp_finite(x))
                x = (x - a.freq_p * ((float) pf_sum[t - begin] / pf_dn)) - a.pres_p * ((float) pm / pf_dn);
        }
        if (a.bias) x = x + b[j];
        if (!((keep >> j) & 1u)) x = -INFINITY;
        v[j] = x;
    }
    if constexpr (sizeof(TO) == 2)
    {
        uint4_t q;
        q.x = half_as_u16((half_t) v[0]) | (half_as_u16((half_t) v[1]) << 16);
        q.y = half_as_u16((half_t) v[2]) | (half_as_u16((half_t) v[3]) << 16);
        q.z = half_as_u16((half_t) v[4]) | (half_as_u16((half_t) v[5]) << 16);
        q.w = half_as_u16((half_t) v[6]) | (half_as_u16((half_t) v[7]) << 16);
        *(uint4_t*) ((half_t*) a.out + (size_t) row * a.ld + c) = q;
    }
    else
    {
        float4_t* p = (float4_t*) ((float*) a.out + (size_t) row * a.ld + c);
        float4_t q0, q1;
        q0.x = v[0]; q0.y = v[1]; q0.z = v[2]; q0.w = v[3]; q1.x = v[4]; q1.y = v[5]; q1.z = v[6]; q1.w = v[7];
        p[0] = q0; p[1] = q1;
    }
}

// (S, D) of one penalty: ranges, the int32 sum, and the bound of the integer frequency sum
static int lp_check_window(const char* what, int S, int D, long long hist, bool sums)
{
    EXL3_CHECK_ARG(S >= 0 && D >= 0, "exl3_logit_process: %s sustain / decay range must not be negative", what);
    EXL3_CHECK_ARG((long long) S + D <= 0x7fffffffll, "exl3_logit_process: %s sustain + decay range must fit an int32", what);
    if (sums)
    {
        const long long cnt = (long long) S + D < hist ? (long long) S + D : hist, dn = D > 0 ? D : 1;
        EXL3_CHECK_ARG(cnt * dn < (1ll << 32), "exl3_logit_process: %s window too large for the integer frequency sum (min(S + D, history) * max(D, 1) must stay below 2^32)", what);
    }
    return EXL3_OK;
}

extern "C" int exl3_logit_process(const void* logits_in, int in_fp32, void* logits_out, int out_fp32, int m, int ld, int size,
                                  const int32_t* past_a, int lda, int len_a, const int32_t* past_b, int ldb, int len_b, const int64_t* len_b_dev, int len_b_bias,
                                  float rep_p, int rep_sustain, int rep_decay, float pres_p, float freq_p, int pf_sustain, int pf_decay,
                                  const float* bias, const uint32_t* bitmask, int bitmask_rows, int bitmask_words, void* stream)
{
    EXL3_CHECK_ARG(m >= 1 && m <= LP_MAX_ROWS, "exl3_logit_process: m must be in [1, 16]");
    EXL3_CHECK_ARG(ld >= 8 && ld % 8 == 0 && size >= 1 && size <= ld, "exl3_logit_process: ld must be a multiple of 8 and 1 <= size <= ld");
    EXL3_CHECK_ARG(logits_in && logits_out, "exl3_logit_process: null pointer");
    EXL3_CHECK_ARG((((uintptr_t) logits_in | (uintptr_t) logits_out) & 15) == 0, "exl3_logit_process: logits must be 16-byte aligned");
    EXL3_CHECK_ARG((in_fp32 == 0 || in_fp32 == 1) && (out_fp32 == 0 || out_fp32 == 1), "exl3_logit_process: the type flags are 0 (fp16) or 1 (fp32)");
    EXL3_CHECK_ARG(logits_in != logits_out || in_fp32 == out_fp32, "exl3_logit_process: in place needs one type on both sides");
    EXL3_CHECK_ARG(len_a >= 0 && (len_a == 0 || (past_a && lda >= len_a)), "exl3_logit_process: past_a needs 0 <= len_a <= lda");
    EXL3_CHECK_ARG(ldb >= 0 && len_b >= 0 && len_b <= ldb, "exl3_logit_process: past_b needs 0 <= len_b <= ldb");
    EXL3_CHECK_ARG(past_b || (ldb == 0 && !len_b_dev), "exl3_logit_process: a length without past_b");
    EXL3_CHECK_ARG((long long) len_a + ldb <= LP_MAX_HIST, "exl3_logit_process: len_a + ldb must not exceed 2^30");
    EXL3_CHECK_ARG(!len_b_dev || ((uintptr_t) len_b_dev & 7) == 0, "exl3_logit_process: the device length must be an aligned int64 word");
    EXL3_CHECK_ARG(!isnan(rep_p) && !isnan(pres_p) && !isnan(freq_p) && !isinf(pres_p) && !isinf(freq_p) && isfinite(rep_p) && rep_p > 0.0f,
                   "exl3_logit_process: rep_p must be positive and finite, pres_p / freq_p finite");
    const long long hist = (long long) len_a + ldb;
    if (int rc = lp_check_window("repetition", rep_sustain, rep_decay, hist, false)) return rc;
    const bool pf_on = (pres_p != 0.0f || freq_p != 0.0f) && (long long) pf_sustain + pf_decay > 0;
    if (int rc = lp_check_window("presence / frequency", pf_sustain, pf_decay, hist, pf_on)) return rc;
    if (bitmask)
    {
        EXL3_CHECK_ARG((bitmask_rows == 1 || bitmask_rows == m) && bitmask_words >= 1, "exl3_logit_process: the bitmask is [1 or m][words >= 1]");
        EXL3_CHECK_ARG(((uintptr_t) bitmask & 3) == 0, "exl3_logit_process: the bitmask must be 4-byte aligned");
    }
    EXL3_CHECK_ARG(!bias || ((uintptr_t) bias & 15) == 0, "exl3_logit_process: the bias must be 16-byte aligned");

    lp_args a;
    a.in = logits_in; a.out = logits_out; a.ld = ld; a.size = size;
    a.past_a = past_a; a.lda = lda; a.len_a = len_a; a.past_b = past_b; a.ldb = ldb; a.len_b = len_b; a.len_b_dev = (const long long*) len_b_dev; a.len_b_bias = len_b_bias;
    // the reference's no-op rules (custom.py:790-793, :855-858)
    a.rep_on = rep_p != 1.0f && (long long) rep_sustain + rep_decay > 0; a.rep_S = rep_sustain; a.rep_D = rep_decay; a.rep_p = rep_p;
    a.pf_on = pf_on; a.pf_S = pf_sustain; a.pf_D = pf_decay; a.pres_p = pres_p; a.freq_p = freq_p;
    a.bias = bias; a.bitmask = bitmask; a.bitmask_row_stride = bitmask && bitmask_rows == m && m > 1 ? bitmask_words : 0; a.bitmask_words = bitmask_words;
    const size_t lds = (size_t) ((a.rep_on ? 1 : 0) + (a.pf_on ? 2 : 0)) * LP_SPAN * sizeof(uint32_t);
    const dim3 grid((ld + LP_SPAN - 1) / LP_SPAN, m);
    hipStream_t st = (hipStream_t) stream;
    if (!in_fp32 && !out_fp32) lp_kernel<half_t, half_t><<<grid, LP_THREADS, lds, st>>>(a);
    else if (!in_fp32)         lp_kernel<half_t, float><<<grid, LP_THREADS, lds, st>>>(a);
    else if (!out_fp32)        lp_kernel<float, half_t><<<grid, LP_THREADS, lds, st>>>(a);
    else                       lp_kernel<float, float><<<grid, LP_THREADS, lds, st>>>(a);
    return exl3_check_launch("logit_process");
}
