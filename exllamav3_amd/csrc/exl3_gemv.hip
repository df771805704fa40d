// EXL3 quantized GEMV / small-m GEMM for gfx950 (decode path):   C = ((A * suh) H) @ dequant(B) H * svh (+ bias)
//
// Host dispatcher + the split-k reduce kernels.  Replaces the reference's cooperative stream-K kernels (quant/exl3_gemv_kernel.cuh:138-402,
// quant/exl3_gemm_kernel.cuh:8-80) with a design that needs no grid sync (a grid sync costs 26 us on MI355X, MI355X_MICROARCH.md
// "barrier-cg"): grid = (n/128 column blocks) x S k-slices; a workgroup owns 128 output columns = one output Hadamard block and a k-slice
// that is a whole number of 128-wide input Hadamard blocks, so BOTH rotations are workgroup-local: the input Hadamard is recomputed per
// workgroup in the prologue from x (L2-resident) and the output Hadamard runs in the epilogue (S == 1), in the split-k reduce kernel below
// (S > 1) or in the consumer of a deferred launch (exl3_glue.hip).  The kernels themselves: exl3_gemv2.kspec.hip (1..16 rows per weight
// pass, column-pair-per-lane decode into v_mfma_f32_4x4x4_16B_f16) and exl3_gemm3.kspec.hip (5..64 rows, 16x16x32 MFMAs fed from the decoding lanes' registers).
// (The first-generation kernel of round 1 -- 4-wave workgroups, 16x16x32 MFMA on B-fragment-ordered lanes -- was an A/B baseline only and
// has been removed; git history has it.)
//
// Variants (VAR):
//   0 EXACT : B operand = the reference's fp16 weights bit-for-bit (one fp16 add / fma per weight).
//   1 FAST  : cb0/cb1 "split": weight = lo + hi (two fp16 halves of the codebook word) is fed to the MFMA as
//             two k-slots against a duplicated activation, skipping the fp16 add and all packing
//             (unrounded lo+hi: closer to exact arithmetic than the reference by <= 2^-12 relative per weight);
//             cb2 "raw": the MFMA multiplies fp16(1024 + bytesum) and the affine map k_inv * acc + k_bias * sum(x)
//             is applied once per output in the epilogue.
#include "exl3_common.cuh"
#include "exl3_api_internal.h"
#include <string.h>
#include <stdlib.h>

#include "exl3_gemv_args.h"

// Split-k reduce + output Hadamard + svh (+ bias).  One half-wave per (row, column block).
__global__ __launch_bounds__(256)
void exl3_gemv_reduce_kernel(const GemvArgs a, int total_colblocks)
{
    const int l = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const int m = a.m;
    const int64_t item = (int64_t) blockIdx.x * 8 + hw;            // (cbg, row)
    const bool act = item < (int64_t) total_colblocks * m;
    const int cbg = act ? (int) (item / m) : 0;
    const int row = act ? (int) (item % m) : 0;
    int mi = 0, cbl, n, ws_off;
    const half_t* svh_m; const half_t* bias_m = nullptr; void* C_m;
    float out_scale = HAD_R_SCALE_128;
    bool skip = false;
    if (a.tbl.B)
    {
        const int slot = cbg / a.tbl.cbs_per_mat;
        const SlotRef_t sr = resolve_slot(a.tbl, slot);
        skip = sr.mat_index < 0;
        cbl = cbg - slot * a.tbl.cbs_per_mat; n = a.tbl.n;
        ws_off = slot * a.tbl.cbs_per_mat * a.S * a.m * 128;
        svh_m = skip ? nullptr : (const half_t*) a.tbl.svh[sr.mat_index];
        C_m = a.c_fp32 ? (void*) ((float*) a.tbl.C + (size_t) slot * a.tbl.c_slot_stride) : (void*) ((half_t*) a.tbl.C + (size_t) slot * a.tbl.c_slot_stride);
        if (a.tbl.n_list && !skip) { n = a.tbl.n_list[sr.mat_index]; C_m = (void*) a.tbl.c_list[sr.mat_index]; skip = cbl >= (n >> 7); }
        out_scale = HAD_R_SCALE_128 * sr.weight;
    }
    else
    {
        #pragma unroll
        for (int i = 1; i < GEMV_MAX_MATS; ++i) if (i < a.num_mats && cbg >= a.mat[i].cb_first) mi = i;
        cbl = cbg - a.mat[mi].cb_first; n = a.mat[mi].n; ws_off = a.mat[mi].ws_offset;
        svh_m = a.mat[mi].svh; bias_m = a.mat[mi].bias; C_m = a.mat[mi].C;
    }
    const float* slab = a.workspace + ws_off + ((size_t) cbl * a.S) * (size_t) m * 128 + (size_t) row * 128;
    float4_t v = { 0.f, 0.f, 0.f, 0.f };
    for (int s = 0; s < a.S; ++s)
    {
        float4_t p = ((const float4_t*) (slab + (size_t) s * m * 128))[l];
        v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    float h0 = v.x, h1 = v.y, h2 = v.z, h3 = v.w;
    had128_f32x4(h0, h1, h2, h3, l);
    h0 *= out_scale; h1 *= out_scale; h2 *= out_scale; h3 *= out_scale;
    if (!act || skip) return;
    const half_t* svh = svh_m + cbl * 128;
    const half_t* bias = bias_m ? bias_m + cbl * 128 : nullptr;
    half4_t sc = ((const half4_t*) svh)[l];
    size_t off = ((size_t) a.c_row_offset + row) * n + cbl * 128 + 4 * l;
    if (a.c_fp32)
    {
        float4_t o = { h0 * (float) sc.x, h1 * (float) sc.y, h2 * (float) sc.z, h3 * (float) sc.w };
        if (bias) { half4_t bv = ((const half4_t*) bias)[l]; o.x += (float) bv.x; o.y += (float) bv.y; o.z += (float) bv.z; o.w += (float) bv.w; }
        *((float4_t*) ((float*) C_m + off)) = o;
    }
    else
    {
        half4_t o = { f2h(h0), f2h(h1), f2h(h2), f2h(h3) };
        o = o * sc;
        if (bias) o = o + ((const half4_t*) bias)[l];
        *((half4_t*) ((half_t*) C_m + off)) = o;
    }
}

// Final step of the weighted (MoE) mgemm: every group of `stride` consecutive slots is summed into output row-block t, in slot order
// (fp16: sequential __hadd from zero, fp32: sequential adds -- quant/exl3_gemm_kernel.cuh:241-290).  With an expert range the in-range slots were
// compacted to the front and only THEY are summed (the reference continues with bszm = the in-range count, exl3_gemm_kernel.cuh:101-127: slots this
// launch never wrote do not enter the sum, no in-range slot at all gives zeros) -- C needs no zero fill.
__global__ void mgemm_slot_reduce_kernel(void* C, int c_fp32, int num_tokens, int stride, int64_t mn, const int64_t* __restrict__ indices, int bszm,
                                         int min_index, int max_index)
{
    const int64_t col = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (min_index >= 0)
    {
        // the in-range slot count is uniform across the launch: one thread of the workgroup counts, the others read it from LDS (every
        // thread used to re-read all bszm indices)
        __shared__ int cnt_s;
        if (threadIdx.x == 0)
        {
            int cnt = 0;
            for (int i = 0; i < bszm; ++i) { const int64_t ix = indices[i]; cnt += (ix >= min_index && ix < max_index) ? 1 : 0; }
            cnt_s = cnt;
        }
        __syncthreads();
        stride = cnt_s;                                              // num_tokens == 1 with an expert range (host-checked)
    }
    if (col >= mn) return;
    for (int t = 0; t < num_tokens; ++t)
    {
        if (c_fp32)
        {
            const float* p = (const float*) C + (int64_t) t * stride * mn + col;
            float sum = 0.0f;
            for (int j = 0; j < stride; ++j) sum += p[(int64_t) j * mn];
            ((float*) C)[(int64_t) t * mn + col] = sum;
        }
        else
        {
            const half_t* p = (const half_t*) C + (int64_t) t * stride * mn + col;
            half_t sum = (half_t) 0.0f;
            for (int j = 0; j < stride; ++j) sum = sum + p[(int64_t) j * mn];
            ((half_t*) C)[(int64_t) t * mn + col] = sum;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Host side: every entry point fills a GemvCall; gemv_run validates it, plans each pass (gemv_plan_pass: pure, also behind the device-free
// exl3_gemv_plan query that tests/test_gemv_plan.py replays), fills the GemvArgs and launches.
// ------------------------------------------------------------------------------------------------

static int g_gemv_variant = -1;      // -1: read EXL3_HIP_GEMV_VARIANT (default 1 = FAST)
static int g_gemv_nwv = 0;           // 0 = heuristic; otherwise cap on waves per workgroup (tuning / tests)
static int g_gemv_defer_wg_per_cu = 0;
// XCD-local tail hand-off (exl3_gemv_resid): OPT-IN.  It is only correct if workgroup i of a 1-D grid runs on XCD i % 8, which HIP does not
// promise (CU masking, harvested XCDs, other firmware): enabling it runs a probe over the grid sizes the mode is used with and refuses
// (EXL3_ERR_ARG, mode stays off) unless every workgroup reported XCC_ID == blockIdx % 8 on several launches.  Default: agent-scope hand-off.
static int g_tail_xcd_local = 0;
__global__ void exl3_xcc_probe_kernel(uint32_t* bad)
{
    if (threadIdx.x == 0)
    {
        uint32_t x; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
        if ((x & 15u) != (blockIdx.x & 7u)) atomicAdd(bad, 1u);
    }
}
extern "C" int exl3_set_tail_xcd_local(int v)
{
    if (!v) { g_tail_xcd_local = 0; return EXL3_OK; }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(0, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
    { exl3_set_error("exl3_set_tail_xcd_local: cannot probe the workgroup -> XCD mapping during graph capture"); return EXL3_ERR_ARG; }
    uint32_t* bad = nullptr;
    EXL3_CHECK_HIP(hipMalloc(&bad, 4), "exl3_set_tail_xcd_local");
    uint32_t h = 0;
    hipError_t e = hipMemset(bad, 0, 4);
    const int grids[] = { 64, 256, 512, 1024, 2048 };
    for (int rep = 0; rep < 3 && e == hipSuccess; ++rep)
        for (int g : grids) exl3_xcc_probe_kernel<<<g, 256>>>(bad);
    if (e == hipSuccess) e = hipMemcpy(&h, bad, 4, hipMemcpyDeviceToHost);
    (void) hipFree(bad);
    EXL3_CHECK_HIP(e, "exl3_set_tail_xcd_local");
    if (h != 0)
    {
        g_tail_xcd_local = 0;
        exl3_set_error("exl3_set_tail_xcd_local: %u probe workgroups did not run on XCD blockIdx %% 8 on this device; the XCD-local hand-off stays off", h);
        return EXL3_ERR_ARG;
    }
    g_tail_xcd_local = 1;
    return EXL3_OK;
}
static int g_gemm3_min_rows = 5;     // passes with at least this many rows take generation 3 (0 = never); raw (unrotated) input: >= 9
extern "C" int exl3_set_gemm3_min_rows(int v) { g_gemm3_min_rows = v; return EXL3_OK; }
// generation 3, 16-row passes: column blocks per workgroup (1, 2 or 4 = 4- / 8- / 16-wave workgroups sharing one activation tile); 0 = cost model
static int g_gemm3_cpw = -1;
static int gemm3_cpw() { if (g_gemm3_cpw < 0) { const char* e = getenv("EXL3_HIP_GEMM3_CPW"); const int v = e ? atoi(e) : 0; g_gemm3_cpw = (v == 1 || v == 2 || v == 4) ? v : 0; } return g_gemm3_cpw; }
extern "C" int exl3_set_gemm3_cpw(int v) { g_gemm3_cpw = (v == 1 || v == 2 || v == 4) ? v : 0; return EXL3_OK; }
// LDS a generation-3 workgroup may use: one 16-wave workgroup per CU, two 8-wave ones, four of 4 waves (160 KB per CU, some left for the runtime)
static int gemm3_lds_budget(int cpw3) { return cpw3 == 4 ? 139264 : (cpw3 == 2 ? 73728 : 36864); }
static int gemm3_chunk_blocks(int mp, int cpw3, int bps, int chunk_bytes)
{
    const int budget = chunk_bytes > 0 ? chunk_bytes : gemm3_lds_budget(cpw3);
    int chunk = (budget / (mp * 2) - 16) / 128;
    if (chunk > 16 * cpw3) chunk = 16 * cpw3;                // the rotated-input copy maps a chunk row onto <= 64 x waves 16-byte pieces (16 per block)
    if (chunk > 32) chunk = 32;
    if (chunk < 1) chunk = 1;
    if (chunk >= bps) return bps;
    // several chunks: every chunk but the last must be a whole number of the kernel's trips (G3_NR = 4 decode steps = 2 Hadamard blocks)
    chunk &= ~1; if (chunk < 2) chunk = 2;
    return chunk;
}
// Cost model of a generation-3 launch at <= 16 rows (us; fitted to tools/gemv_timeline.py at batch 16, round 4): `groups` workgroup columns of cpw3
// column blocks, s k-slices of b Hadamard blocks.  A wave alone on its SIMD needs ~250 ns per decode step (4 tile rows x 32 columns), w waves sharing a
// SIMD ~{250, 202, 190, 181} ns of SIMD time per step (issue-bound from 2 waves); a CU holds 4 / cpw3 workgroups; a round of workgroups pays ~1.5 us
// before it streams (launch, first rows, activation tile) and a slab per slice is written and read again.
static double gemm3_cost(int groups, int cpw3, int s, int b, int cus, bool deferred)
{
    // (w = 4 above the issue-bound figure: with four waves per SIMD the launch's first microseconds -- every workgroup staging its activation tile behind
    // everyone's first weight rows -- stretch to 3..12 us; sweep of the whole step, tools/r4_g3_sweep.sh: q|k|v 8 / gate|up 2 / down 16 slices at two
    // column blocks per workgroup 70.9 us per layer against 74.9 for the round-3 choices; 16-wave workgroups measured 10 % slower than 8-wave ones)
    static const double tw[5] = { 0.0, 0.250, 0.202, 0.195, 0.210 };
    const long wgs = (long) groups * s;
    const int cap = 4 / cpw3;
    const long rounds = (wgs + (long) cus * cap - 1) / ((long) cus * cap);
    long per_cu = (wgs + cus - 1) / cus; if (per_cu > cap) per_cu = cap;
    const int w = (int) per_cu * cpw3;
    const double t_round = 1.5 + 2.0 * b * w * tw[w] * (cpw3 == 4 ? 1.25 : 1.0);
    return rounds * t_round + 0.03 * s + ((s > 1 && !deferred) ? 5.0 : 0.0);
}

extern "C" int exl3_set_gemv_defer_wg_per_cu(int v) { g_gemv_defer_wg_per_cu = v; return EXL3_OK; }
extern "C" int exl3_set_gemv_max_waves(int v) { g_gemv_nwv = v; return EXL3_OK; }

// generation 4 (exl3_gemv4.kspec.hip) takes the 1..4-row launches it supports (plain / rotated / RMSNorm / silu-mul input, final or deferred
// output, slices of at most 32 Hadamard blocks); 0 pins generation 2 (A/B runs, the bit-identity tests between generation-2 pipelines)
static int g_gemv_gen4 = -1;
static int gemv_gen4()
{
    if (g_gemv_gen4 < 0) { const char* e = getenv("EXL3_HIP_GEMV_GEN4"); g_gemv_gen4 = e ? (atoi(e) != 0) : 1; }
    return g_gemv_gen4;
}
extern "C" int exl3_set_gemv_gen4(int v) { g_gemv_gen4 = v ? 1 : 0; return EXL3_OK; }

// fx pipeline: exl3_fx_zero_next(ptr, bytes) asks the NEXT dispatcher call OF THIS THREAD ON THIS DEVICE to clear a buffer as a side job (the gate / up
// accumulators, cleared by the o_proj launch in front of the gate|up launch that adds into them).  The request is one-shot and never outlives that
// call: gemv_run takes it on entry (take_fx_zero), so an argument error, a launch that is not a plain generation-4 launch, or a launch on another
// device fails loudly ("cannot clear") instead of leaving the pointer armed for an unrelated later launch.
struct FxZeroReq { void* ptr; int64_t bytes; int device; };
static thread_local FxZeroReq g_fx_zero = { nullptr, 0, -1 };
extern "C" int exl3_fx_zero_next(void* ptr, int64_t bytes)
{
    g_fx_zero = FxZeroReq{ nullptr, 0, -1 };
    EXL3_CHECK_ARG(!ptr || (bytes > 0 && bytes % 16 == 0 && (uintptr_t) ptr % 16 == 0 && bytes / 16 < (1ll << 31)), "exl3_fx_zero_next: 16-byte aligned pointer and size");
    if (!ptr) return EXL3_OK;
    int dev = -1;
    EXL3_CHECK_HIP(hipGetDevice(&dev), "exl3_fx_zero_next");
    g_fx_zero = FxZeroReq{ ptr, bytes, dev };
    return EXL3_OK;
}
static FxZeroReq take_fx_zero() { const FxZeroReq r = g_fx_zero; g_fx_zero = FxZeroReq{ nullptr, 0, -1 }; return r; }

static int gemv_variant()
{
    if (g_gemv_variant < 0)
    {
        const char* e = getenv("EXL3_HIP_GEMV_VARIANT");
        g_gemv_variant = e ? atoi(e) : 1;
        if (g_gemv_variant != 0) g_gemv_variant = 1;
    }
    return g_gemv_variant;
}
extern "C" int exl3_set_gemv_variant(int v) { g_gemv_variant = v ? 1 : 0; return EXL3_OK; }

// The knobs as ONE call sees them: snapshotted at the top of the call (and of the plan query), so the planner never reads the globals
struct GemvTuning { int variant, max_waves, defer_wg_per_cu, gemm3_min_rows, gemm3_cpw, gen4, tail_xcd_local, gemm3_chunk_bytes; };
static GemvTuning gemv_tuning()
{
    static const int chunk_bytes_env = [] { const char* e = getenv("EXL3_HIP_GEMM3_CHUNK_BYTES"); return e ? atoi(e) : 0; }();
    GemvTuning t;
    t.variant = gemv_variant(); t.max_waves = g_gemv_nwv; t.defer_wg_per_cu = g_gemv_defer_wg_per_cu; t.gemm3_min_rows = g_gemm3_min_rows;
    t.gemm3_cpw = gemm3_cpw(); t.gen4 = gemv_gen4(); t.tail_xcd_local = g_tail_xcd_local; t.gemm3_chunk_bytes = chunk_bytes_env;
    return t;
}

// The per-K translation units' entry points, indexed by K - 1
#define GEMV_PER_K(f) { f##1, f##2, f##3, f##4, f##5, f##6, f##7, f##8 }
typedef void (*GemvLaunchFn)(int, int, int, int, dim3, size_t, hipStream_t, const GemvArgs&);
static const GemvLaunchFn g_launch_gen2[8] = GEMV_PER_K(exl3_gemv2_launch_k);      // (cb, var, ng, nwv, ...)
static const GemvLaunchFn g_launch_gen3[8] = GEMV_PER_K(exl3_gemm3_launch_k);      // (cb, mt, var, nwt, ...)
static const GemvLaunchFn g_launch_gen4[8] = GEMV_PER_K(exl3_gemv4_launch_k);      // (cb, var, mode, nwv, ...)
static int (* const g_gemm3_max_waves[8])(int mt, int rot) = GEMV_PER_K(exl3_gemm3_max_waves_k);
#undef GEMV_PER_K

// generations 2 and 4: the requested split (fs > 0) or generation 2's own rule, normalised so that no slice is empty
static int choose_split(int total_colblocks, int k, int num_cus, int fs)
{
    const int nb = k / 128;
    int S;
    if (fs > 0) S = fs;
    // gen 2: a workgroup is up to 16 waves that split its k-slice, so one workgroup per CU already fills the CU.
    // Split k across workgroups only until every CU has one (no reduce launch when the column blocks suffice).
    else if (4 * total_colblocks >= 3 * num_cus) S = 1;
    else S = (num_cus + total_colblocks - 1) / total_colblocks;
    if (S < 1) S = 1;
    if (S > nb) S = nb;
    const int blocks_per_slice = (nb + S - 1) / S;
    return (nb + blocks_per_slice - 1) / blocks_per_slice;
}

// GEMV_IN_RESID operands: the producer linear's deferred slabs + svh, and where the workgroups of column block 0 publish the new residual
struct GemvResidIn { const float* slab; int S; const void* svh; void* resid_out; float* ss_out; };

// One request to the dispatcher.  Entry points zero-initialise it (GemvCall c = {}) and assign the fields they use.
struct GemvCall
{
    const void* A; const void* const* Bs; void* const* Cs; const void* const* suhs; const void* const* svhs; const void* const* biases;
    const int* ns; int count, m, k, K, cb, c_fp32, force_split, flags;
    const void* const* xhs; const float* const* xsums;          // GEMV_IN_ROTATED
    float** slabs_out; int* S_out;
    const GemvEpi* epi; const GemvTable* tbl; const GemvResidIn* rsd; const GemvRescale* act_rs; const GemvAttm* attm; const GemvQkvm* qkvm;
    const void* norm_w; const float* ss_part; float eps;        // GEMV_IN_NORM
    const float* act_g; const float* act_u; int act_S; const void* act_svh_g; const void* act_svh_u;      // GEMV_IN_ACT / GEMV_IN_ACTFX
    int cpw;                    // > 0: wave-per-column-block layout (exl3_gemv2.kspec.hip): cpw column blocks of one matrix per workgroup, one wave each
    float* fx_ss_out;           // GEMV_IN_FX
    hipStream_t stream;
};

// What gemv_validate keeps of a request for the planner: sizes, modes and which operands are there -- no device pointer
struct GemvShape
{
    int flags;                  // the request's flags and those its operand blocks imply
    int count, m, k, K, cb, force_split, cpw, total_cb, epi_mode;
    const int* ns;
    bool deferred /* slabs or atomic adds: nothing to reduce */, atomic_out, rotated, in_norm, in_act, in_fx;
    bool tbl, tbl_gen2 /* fp16 act input / per-matrix widths: generation 2's */, rsd, attm, qkvm, xsums /* every matrix has its block sums */, fx_zero;
};

// What one pass launches: one int32 record of exl3_gemv_plan, in this order
struct GemvPlan
{
    int rows;                   // rows of the pass
    int gen;                    // kernel generation 2 | 3 | 4
    int sel;                    // its instantiation: generation 4 mode 0..9, generation 2 ng (rows / 4: 1 | 2 | 4), generation 3 mt (row tiles: 1 | 2 | 4)
    int pre_xh;                 // generation 3: the activations are rotated once in front of the launch
    int S, bps;                 // k-slices, Hadamard blocks per slice
    int nwv;                    // waves per workgroup
    int chunk_blocks;           // generations 2, 3: Hadamard blocks of activations in LDS at a time
    int cpw;                    // column blocks per workgroup: the wave-per-column-block layout's, generation 3's; 0 otherwise
    int grid_x, grid_y, grid_z, lds;
    int ws_floats;              // slab (+ tail epilogue) floats of the pass in the workspace region
    int rows_per_pass, xcd_local;      // GemvEpi
    int reduce;                 // the split-k reduce launch follows
};
static_assert(sizeof(GemvPlan) == EXL3_GEMV_PLAN_INTS * 4, "GemvPlan is the record of exl3_gemv_plan");

static int gemv_validate(const GemvCall& c, bool fx_zero, GemvShape& s)
{
    const void* A = c.A; const void* const* Bs = c.Bs; void* const* Cs = c.Cs; const void* const* suhs = c.suhs; const void* const* svhs = c.svhs;
    const int* ns = c.ns; const int count = c.count, m = c.m, k = c.k, K = c.K, cb = c.cb, cpw = c.cpw, act_S = c.act_S;
    const void* const* xhs = c.xhs; const float* const* xsums = c.xsums; const void* norm_w = c.norm_w; const float* ss_part = c.ss_part;
    const GemvEpi* epi = c.epi; const GemvTable* tbl = c.tbl; const GemvResidIn* rsd = c.rsd; const GemvAttm* attm = c.attm; const GemvQkvm* qkvm = c.qkvm;
    const float* act_g = c.act_g; const float* act_u = c.act_u; const void* act_svh_g = c.act_svh_g; const void* act_svh_u = c.act_svh_u;
    float* fx_ss_out = c.fx_ss_out;
    int flags = c.flags;
    if (rsd) flags |= GEMV_IN_RESID;
    // cpw > 0: wave-per-column-block layout (exl3_gemv2.kspec.hip): cpw column blocks of one matrix per workgroup, one wave each
    EXL3_CHECK_ARG(cpw >= 0 && cpw <= 16, "exl3_gemv_ex: column blocks per workgroup must be in [0, 16]");
    EXL3_CHECK_ARG(!rsd || cpw > 0, "exl3_gemv_ex_resid: needs the wave-per-column-block layout (cpw >= 1)");
    EXL3_CHECK_ARG(cpw == 0 || ((flags & GEMV_OUT_DEFERRED) && m <= 4 && !tbl && !epi && !(flags & GEMV_IN_ROTATED)),
                   "exl3_gemv_ex (cpw): wave-per-column-block launches are deferred, m <= 4, raw / resid / act input");
    if (act_g) flags |= GEMV_IN_ACT;
    if (attm) flags |= GEMV_IN_ATTM;
    EXL3_CHECK_ARG(!attm || (attm->part && attm->nsplit >= 1 && (attm->hd == 128 || attm->hd == 64) && attm->nsplit <= (attm->hd == 128 ? 32 : 16) && attm->gq >= 1 && attm->blocks >= 1
                             && count == 1 && m <= 4 && !tbl && !epi && cpw == 0 && !rsd && !act_g && !(flags & (GEMV_IN_ROTATED | GEMV_IN_NORM))
                             && k == attm->gq * attm->blocks * 128),
                   "exl3_gemv_ex_attm: one matrix, m <= 4, at most 32 (head_dim 128) / 16 (head_dim 64) context splits, k = heads_q x head_dim");
    if (qkvm) flags |= GEMV_IN_QKVM;
    EXL3_CHECK_ARG(!qkvm || (qkvm->sq && qkvm->sk && qkvm->sv && qkvm->S >= 1 && qkvm->svh_q && qkvm->svh_k && qkvm->svh_v && qkvm->rope_sin && qkvm->rope_cos && qkvm->slots
                             && qkvm->k_cache && qkvm->k_scales && qkvm->v_cache && qkvm->v_scales && (qkvm->hd == 64 || qkvm->hd == 128) && qkvm->kvb >= 1
                             && (qkvm->rope_mode == 1 || qkvm->rope_mode == 2) && count == 1 && m <= 4 && !tbl && !epi && cpw == 0 && !rsd && !act_g && !attm
                             && !(flags & (GEMV_IN_ROTATED | GEMV_IN_NORM))),
                   "exl3_gemv_ex_qkvm: one matrix, m <= 4, the q|k|v slabs + scales, the rope tables and cache rows of exl3_qkv_prep, a 4-bit cache");
    if (epi) flags |= GEMV_OUT_DEFERRED;
    // GEMV_OUT_ATOMIC (generation 4): no slabs, every workgroup adds its share of the output into the fixed-point accumulator Cs[i]; like a deferred
    // launch it keeps every workgroup resident (the split is chosen the same way) and it needs svhs
    const bool atomic_out = (flags & GEMV_OUT_ATOMIC) != 0, in_fx = (flags & GEMV_IN_FX) != 0;
    EXL3_CHECK_ARG(!atomic_out || (!(flags & GEMV_OUT_DEFERRED) && ((Cs && svhs) || (tbl && tbl->C && tbl->svh && tbl->slots_per_token >= 1)) && m <= 4 && !epi && cpw == 0 && !rsd),
                   "exl3_gemv_ex: GEMV_OUT_ATOMIC needs the accumulators (Cs), svhs, m <= 4 and excludes GEMV_OUT_DEFERRED");
    EXL3_CHECK_ARG(!in_fx || ((flags & GEMV_IN_NORM) && m <= 4 && fx_ss_out), "exl3_gemv_ex_fx: needs GEMV_IN_NORM, m <= 4 and ss_out");
    const bool deferred = (flags & (GEMV_OUT_DEFERRED | GEMV_OUT_ATOMIC)) != 0, rotated = (flags & GEMV_IN_ROTATED) != 0;
    EXL3_CHECK_ARG(!(deferred || rotated) || m <= 16, "exl3_gemv_ex: at most 16 rows");
    EXL3_CHECK_ARG(!rotated || xhs, "exl3_gemv_ex: rotated input requires xh pointers");
    const bool in_norm = (flags & GEMV_IN_NORM) != 0;
    EXL3_CHECK_ARG(!in_norm || (norm_w && ss_part && !rotated && m <= 16), "exl3_gemv_ex: GEMV_IN_NORM needs norm_w, ss_part, raw input and m <= 16");
    EXL3_CHECK_ARG(count >= 1 && (tbl || count <= GEMV_MAX_MATS), "exl3_mgemm: between 1 and %d matrices per launch", GEMV_MAX_MATS);
    EXL3_CHECK_ARG(!tbl || (m <= 16 && !rotated && !epi), "exl3_mgemm (indexed): at most 16 rows per slot");
    EXL3_CHECK_ARG(K >= 1 && K <= 8, "exl3_gemm: K must be in [1, 8]");
    EXL3_CHECK_ARG(cb >= 0 && cb <= 2, "exl3_gemm: bad codebook");
    EXL3_CHECK_ARG(k % 128 == 0 && k > 0, "exl3_gemm: k must be divisible by 128");
    EXL3_CHECK_ARG(m >= 1, "exl3_gemm: m must be >= 1");
    const bool in_act = (flags & GEMV_IN_ACT) != 0;
    EXL3_CHECK_ARG(!in_act || (act_g && act_u && ((act_svh_g && act_svh_u && count == 1) || (tbl && tbl->act_svh)) && act_S >= 1 && !rotated && m <= 4),
                   "exl3_gemv_ex_act: needs gate / up slabs + svh, one matrix, m <= 4");
    EXL3_CHECK_ARG(A || rotated || in_act || attm || qkvm, "exl3_gemm: null A");
    EXL3_CHECK_ARG(!rsd || (in_norm && deferred && m <= 4 && rsd->slab && rsd->S >= 1 && rsd->svh && rsd->resid_out && rsd->ss_out && rsd->resid_out != A),
                   "exl3_gemv_ex_resid: needs GEMV_IN_NORM, deferred output, m <= 4, producer slabs + svh and a resid_out buffer other than resid_in");
    int total_cb = 0;
    bool has_xsums = xsums != nullptr;
    if (tbl)
    {
        EXL3_CHECK_ARG(ns[0] % 128 == 0 && ns[0] > 0, "exl3_gemm: n must be divisible by 128");
        total_cb = count * (ns[0] / 128);
    }
    for (int i = 0; i < (tbl ? 0 : count); ++i)
    {
        EXL3_CHECK_ARG(ns[i] % 128 == 0 && ns[i] > 0, "exl3_gemm: n must be divisible by 128");
        EXL3_CHECK_ARG(Bs[i] && (deferred || (Cs && Cs[i] && svhs && svhs[i])) && (rotated || (suhs && suhs[i])), "exl3_gemm: null pointer");
        EXL3_CHECK_ARG(!atomic_out || (Cs[i] && svhs[i]), "exl3_gemv_ex: GEMV_OUT_ATOMIC needs an accumulator and svh per matrix");
        total_cb += ns[i] / 128;
        if (has_xsums && !xsums[i]) has_xsums = false;
    }
    s.flags = flags; s.count = count; s.m = m; s.k = k; s.K = K; s.cb = cb; s.force_split = c.force_split; s.cpw = cpw; s.total_cb = total_cb;
    s.epi_mode = epi ? epi->mode : GEMV_EPI_NONE; s.ns = ns;
    s.deferred = deferred; s.atomic_out = atomic_out; s.rotated = rotated; s.in_norm = in_norm; s.in_act = in_act; s.in_fx = in_fx;
    s.tbl = tbl != nullptr; s.tbl_gen2 = tbl && (tbl->act_u || tbl->n_list); s.rsd = rsd != nullptr; s.attm = attm != nullptr; s.qkvm = qkvm != nullptr;
    s.xsums = has_xsums; s.fx_zero = fx_zero;
    return EXL3_OK;
}

// generation 3 streams the weights once per up to 64 rows (exl3_gemm3.kspec.hip); the special input / output modes stay on generation 2
static bool gemm3_admits(const GemvShape& s, const GemvTuning& t) { return t.gemm3_min_rows > 0 && !s.in_norm && !s.tbl && !s.in_act && s.epi_mode == GEMV_EPI_NONE; }
static int gemv_pass_rows(const GemvShape& s, const GemvTuning& t) { return (gemm3_admits(s, t) && !s.deferred && !s.rotated && s.m > 16) ? (s.m > 32 ? 64 : 32) : 16; }

// generation 3: the cheapest normalised split (no empty slice) by the cost model, for `groups` workgroup columns of cpw3 column blocks each
static int gemm3_cost_split(const GemvShape& s, int mp, int cus, int cpw3, int groups)
{
    const int nbk = s.k / 128;
    int forced_S = 0;
    if (s.force_split > 0)
    {
        const int fsq = s.force_split > nbk ? nbk : (s.force_split > 64 ? 64 : s.force_split);        // (the search below stops at 64 slices)
        const int fb = (nbk + fsq - 1) / fsq; forced_S = (nbk + fb - 1) / fb;
    }
    double best = 1e30;
    int S = 1;                                              // (forced split that is not normalised / nothing fits: one slice)
    for (int s_ = 1; s_ <= nbk && s_ <= 64; ++s_)
    {
        const int b = (nbk + s_ - 1) / s_;
        if ((nbk + b - 1) / b != s_) continue;          // not a normalised split
        if (forced_S > 0 && s_ != forced_S) continue;
        // the slabs must fit one workspace region -- a launch that writes none (one slice, finished output) always fits (with
        // every candidate rejected the split stayed 0 and the slice length below divided by it: lm_head-sized n at 33..64 rows)
        if ((s_ > 1 || s.deferred) && (long) s.total_cb * s_ * mp * 512 > (long) EXL3_WS_REGION_BYTES) continue;
        const double c = gemm3_cost(groups, cpw3, s_, b, cus, s.deferred);
        if (c < best) { best = c; S = s_; }
    }
    return S;
}
// deferred epilogue: the reduction is free (a glue kernel / tail epilogue does it), so pick the split that balances the
// chip.  All workgroups of these launches are resident at once and the kernel is VALU-bound per CU, so the launch
// takes as long as the busiest CU: ceil(workgroups / CUs) * blocks per workgroup.  Fewest slabs among the minima;
// a light preference for >= 2 workgroups per CU (tools/sweep_split.py: gate/up 3 -> 8 is -3 us per layer).
static int deferred_balance_split(const GemvShape& s, int cus, const GemvTuning& t)
{
    const int nbk = s.k / 128;
    double best_cost = 1e30;
    int fs = 1;
    for (int sp = 1; sp <= nbk && sp <= 64; ++sp)
    {
        const int b = (nbk + sp - 1) / sp;
        if ((nbk + b - 1) / b != sp) continue;              // not a normalised split
        const long wg = (long) s.total_cb * sp;
        const double cost = (double) ((wg + cus - 1) / cus) * b + (wg < 2l * cus ? 0.25 : 0.0) + 1e-3 * sp;
        if (cost < best_cost) { best_cost = cost; fs = sp; }
    }
    if (t.defer_wg_per_cu > 0) fs = (t.defer_wg_per_cu * cus + s.total_cb - 1) / s.total_cb;
    if (fs < 1) fs = 1;
    if (s.epi_mode != GEMV_EPI_NONE && fs > 64) fs = 64;     // tail epilogue: one pass of slabs must fit the workgroup LDS
    return fs;
}
// waves per workgroup, generation 4: generation 2's measured choices (below) within 8 waves
static int gemv4_waves(int bps, bool deferred, int max_waves)
{
    int nwv = 8;
    if (nwv > (bps > 4 ? bps : 4)) nwv = bps > 4 ? bps : 4;
    if (deferred && nwv > 4 && bps <= 16) nwv = 4;
    if (max_waves < 0) nwv = -max_waves < 8 ? -max_waves : 8;
    if (nwv > bps * 4) nwv = bps * 4;
    if (max_waves > 0 && nwv > max_waves) nwv = max_waves;
    return nwv < 1 ? 1 : nwv;
}
// waves per workgroup, generation 2 (classic layout; the wave-per-column-block layout has one wave per column block of the group)
static int gemv2_waves(const GemvShape& s, int ng, int bps, int max_waves)
{
    int nwv = 16 / ng;                                   // partial-sum LDS: nwv * 4*ng rows * 512 B <= 32 KB
    const int units = bps * (8 / G2_PF);                 // the waves split the slice's tile rows in units of G2_PF
    // measured on MI355X (tools/prof_tail.py, batch 1): one wave per Hadamard block of the slice, but at least 4 waves --
    // more waves than that do not help (the kernel is VALU / fixed-latency bound), fewer starve the short slices
    if (nwv > (bps > 4 ? bps : 4)) nwv = bps > 4 ? bps : 4;
    // deferred launches keep every workgroup resident (balanced split above): 4 waves = one per SIMD per workgroup with equal
    // rows each, so no SIMD ends up with an extra wave (tools/gemv_timeline.py: down_proj's 7-wave workgroups left a
    // 4/4/3/3 SIMD load and a 1.8 us wait at the workgroup barrier)
    if (s.deferred && nwv > 4 && bps <= 16) nwv = 4;
    // variants above 64 VGPRs (3INST/MCG decode, NORM prep, K >= 5 rings) fit 7 or 6 waves per SIMD: three 8-wave workgroups per
    // CU instead of one 16-wave workgroup (tools/bench_lmhead.py: lm_head 3INST 105 -> 87 us, NORM 92 -> 81 us)
    if (!s.deferred && ng == 1 && (s.cb != 2 || s.tbl || s.K >= 5) && nwv > 8) nwv = 8;
    if (max_waves < 0) nwv = (-max_waves < 16 / ng) ? -max_waves : 16 / ng;      // tuning: forced wave count
    if (s.in_act && nwv > 4) nwv = 4;                    // (classic layout) ACT-mode kernels are built for 4-wave workgroups (256 VGPRs available)
    if (nwv > units) nwv = units;
    if (max_waves > 0 && nwv > max_waves) nwv = max_waves;
    return nwv < 1 ? 1 : nwv;
}

// Everything one pass of mp rows launches on a chip of num_cus CUs.  Pure: no HIP call, no context, no pointer is followed but s.ns.
static int gemv_plan_pass(const GemvShape& s, int mp, int num_cus, const GemvTuning& t, GemvPlan& p)
{
    memset((void*) &p, 0, sizeof(p));
    const int k = s.k, nb = k / 128, cpw = s.cpw, count = s.count, var = t.variant;
    const bool epi = s.epi_mode != GEMV_EPI_NONE;
    p.rows = mp;
    // measured in the fused pipeline (tools/prof_tail.py, Llama-3.1-8B shapes): generation 3 is ahead from 5 rows with rotated input; with raw
    // input its 8 half-waves per workgroup would spend longer on the input Hadamards than generation 2's 16..32, so it starts at 9 rows
    // and, for wide launches, rotates the activations ONCE first (the role of the reference's A_had temporary, "storage for input transform": quant/exl3_gemm.cu:30, 139-145)
    const bool g3 = cpw == 0 && gemm3_admits(s, t) && mp >= (s.rotated ? t.gemm3_min_rows : (t.gemm3_min_rows > 9 ? t.gemm3_min_rows : 9));
    p.pre_xh = g3 && !s.rotated && (long) s.total_cb * mp >= 1024 && (size_t) mp * k * 2 * count <= (size_t) EXL3_WS_XH_BYTES;
    const bool rot_pass = s.rotated || p.pre_xh;
    int groups = s.total_cb;                                   // workgroup columns of the grid
    if (g3)
    {
        // generation 3: column blocks per workgroup and the split are chosen together (16-row passes; 32- / 64-row passes keep 4-wave workgroups):
        // two column blocks per workgroup wherever the instantiation's register budget allows 8 waves (measured best in the whole step; one block
        // otherwise; four only on request: exl3_set_gemm3_cpw / EXL3_HIP_GEMM3_CPW) -- the split then follows the cost model for that choice
        p.sel = mp > 32 ? 4 : (mp > 16 ? 2 : 1);
        const int maxw = g_gemm3_max_waves[s.K - 1](p.sel, rot_pass ? 1 : 0);
        p.cpw = (t.gemm3_cpw && 4 * t.gemm3_cpw <= maxw) ? t.gemm3_cpw : (maxw >= 8 ? 2 : 1);
        groups = 0;
        for (int i = 0; i < count; ++i) groups += (s.ns[i] / 128 + p.cpw - 1) / p.cpw;
        p.S = gemm3_cost_split(s, mp, num_cus, p.cpw, groups);
    }
    else
    {
        int fs = s.force_split;
        if (cpw > 0)
        {
            p.cpw = cpw;
            groups = 0;
            for (int i = 0; i < count; ++i) groups += (s.ns[i] / 128 + cpw - 1) / cpw;
            if (fs == 0)
            {
                // default: about 16 waves per CU in all (4 per SIMD at this layout's 128 VGPRs); tuned values come from the caller
                long want = ((long) num_cus * 16 + (long) groups * cpw - 1) / ((long) groups * cpw);
                if (want < 1) want = 1;
                if (want > nb) want = nb;
                fs = (int) want;
            }
        }
        else if (s.deferred && fs == 0) fs = deferred_balance_split(s, num_cus, t);
        p.S = choose_split(s.total_cb, k, num_cus, fs);
    }
    const int S = p.S;
    EXL3_CHECK_ARG(S >= 1, "exl3_gemm: internal: split factor %d", S);
    const int bps = p.bps = (nb + S - 1) / S;
    int64_t wso = (int64_t) s.total_cb * S * mp * 128;         // slabs [column block][S][mp][128] of every matrix / slot
    if (epi)
    {
        if (s.epi_mode == GEMV_EPI_NORM) wso += (int64_t) mp * (s.ns[0] / 128);      // + [mp][n/128] sums of squares
        // one XCD per column block needs (column blocks x S) / 8 consecutive logical workgroups to hold whole column blocks
        p.xcd_local = (s.epi_mode == GEMV_EPI_RESID && t.tail_xcd_local && s.total_cb % 8 == 0) ? 1 : 0;
        EXL3_CHECK_ARG(s.total_cb + 1 <= EXL3_NUM_TICKETS, "exl3_gemv: too many column blocks for the ticket table");
        EXL3_CHECK_ARG(S <= 128, "exl3_gemv: split too deep for the tail epilogue");
    }
    EXL3_CHECK_ARG((S == 1 && !s.deferred) || s.atomic_out || wso * 4 <= EXL3_WS_REGION_BYTES, "exl3_gemm: split-k workspace too small");
    p.ws_floats = (int) wso;
    p.reduce = S > 1 && !s.deferred;                         // (GEMV_OUT_ATOMIC launches count as deferred: nothing to reduce)
    const int ng = mp <= 4 ? 1 : (mp <= 8 ? 2 : 4);
    // generation 4: table launches (MoE) with raw-x / slab-act inputs -- the fp16 gate / up act input and per-matrix widths stay generation 2's;
    // the mul1 FAST variant needs the producer's block sums with rotated input
    const bool g4 = !g3 && t.gen4 && ng == 1 && !s.tbl_gen2 && !epi && cpw == 0 && !s.rsd && bps <= 32 && !(rot_pass && var == 1 && s.cb == 2 && !s.xsums);
    p.gen = g3 ? 3 : (g4 ? 4 : 2);
    EXL3_CHECK_ARG(!s.fx_zero || g4, "exl3_fx_zero_next: the launch that followed cannot clear the buffer (not a generation-4 launch: rows > 4, a slice of more than 32 Hadamard blocks, a tail / wave-per-column-block mode, or generation 4 switched off)");
    // 2-D grid (k-slices, column blocks or groups): dispatched x-fastest, i.e. in the order column block * S + slice; the kernels read
    // their pair from blockIdx instead of dividing a linear id
    p.grid_x = S; p.grid_y = groups; p.grid_z = 1;
    if (g3)
    {
        // workgroup = 4 cpw waves = cpw adjacent column blocks of one matrix sharing ONE activation tile in LDS (16 rows keep a whole 8-block
        // slice resident at 4 waves, a whole k = 4096 at 16: one chunk, no second prologue / barrier inside the stream)
        p.nwv = 4 * p.cpw;
        p.chunk_blocks = gemm3_chunk_blocks(mp, p.cpw, bps, t.gemm3_chunk_bytes);
        p.lds = (int) exl3_gemm3_lds_bytes(mp, p.chunk_blocks, p.nwv);
    }
    else if (g4)
    {
        p.sel = s.qkvm ? 9 : s.attm ? 8 : s.tbl ? (s.in_act ? 7 : 6) : s.in_act ? ((s.flags & GEMV_IN_ACTFX) ? 5 : 3) : (s.in_norm ? (s.in_fx ? 4 : 2) : (rot_pass ? 0 : 1));
        p.nwv = gemv4_waves(bps, s.deferred, t.max_waves);
        p.lds = (int) exl3_gemv4_lds_bytes(p.sel, p.nwv, mp, bps);
    }
    else
    {
        EXL3_CHECK_ARG(!s.atomic_out && !s.in_fx && !s.attm && !s.qkvm && !(s.flags & GEMV_IN_ACTFX) && !(s.tbl && s.in_act), "exl3_gemv_ex: GEMV_OUT_ATOMIC / GEMV_IN_FX / GEMV_IN_ACTFX / GEMV_IN_ATTM / GEMV_IN_QKVM / slab-act table launches are generation-4 launches (m <= 4, slices of <= 32 Hadamard blocks, generation 4 enabled)");
        p.sel = ng;
        p.nwv = cpw > 0 ? cpw : gemv2_waves(s, ng, bps, t.max_waves);
        // activation fragments of one chunk of Hadamard blocks, built once per workgroup: up to ~48 KB, the whole slice when it fits
        const int AHh = (var == 1 && s.cb != 2) ? 32 : 16;
        int chunk = (int) ((size_t) 49152 / ((size_t) 8 * mp * AHh * 2));
        if (chunk < 1) chunk = 1;
        if (chunk > bps) chunk = bps;
        EXL3_CHECK_ARG(cpw == 0 || chunk >= bps, "exl3_gemv_ex (cpw): the slice's activation fragments must fit one LDS chunk (use a deeper split)");
        p.chunk_blocks = chunk;
        size_t lds = exl3_gemv2_lds_bytes(ng, var, s.cb, p.nwv, mp, chunk);
        if (epi)
        {
            // tail epilogue: the last workgroup of a column block stages rows_per_pass rows x sets x S slab lines (512 B) in LDS
            const size_t line_bytes = (size_t) (s.epi_mode == GEMV_EPI_ACT ? 2 : 1) * S * 512;
            if (lds < line_bytes) lds = line_bytes;
            int rpp = (int) (lds / line_bytes);
            if (rpp > mp) rpp = mp;
            if (rpp > 2 * p.nwv) rpp = 2 * p.nwv;
            p.rows_per_pass = rpp;
        }
        p.lds = (int) lds;
    }
    EXL3_CHECK_ARG(groups <= 65535, "exl3_gemm: too many column blocks for one launch");
    if (g4 && s.tbl)
    {
        EXL3_CHECK_ARG(count <= 65535, "exl3_mgemm: too many slots for one launch");
        p.grid_y = s.ns[0] / 128; p.grid_z = count;          // (k-slices, column blocks of one matrix, slots)
    }
    return EXL3_OK;
}

// Pointer and offset bookkeeping of one pass: the kernels' argument block, its workspace region (slab-writing launches alternate between two),
// the slab addresses handed back, the fx-zero hand-over.  pre_xh[i]: matrix i's activations rotated in front of the launch (p.pre_xh), else null.
static int gemv_fill_args(const GemvCall& c, const GemvShape& s, const GemvPlan& p, int m0, Exl3DevCtx* ctx, const void* const* pre_xh,
                          const FxZeroReq& fxz, GemvArgs& args)
{
    memset((void*) &args, 0, sizeof(args));
    const int mp = p.rows, nmat = c.tbl ? 0 : c.count;
    if (fxz.ptr)
    {
        int dev_now = -1;
        EXL3_CHECK_HIP(hipGetDevice(&dev_now), "exl3_gemv_ex");
        EXL3_CHECK_ARG(!c.tbl && dev_now == fxz.device, "exl3_fx_zero_next: the launch that follows must be a plain (non-table) generation-4 launch on the device the request was made on");
        args.fx_zero = fxz.ptr; args.fx_zero_n16 = (int) (fxz.bytes / 16);
    }
    args.act_g = c.act_g; args.act_u = c.act_u; args.act_S = c.act_S;
    args.act_svh_g = (const half_t*) c.act_svh_g; args.act_svh_u = (const half_t*) c.act_svh_u;
    args.norm_w = (const half_t*) c.norm_w; args.ss_part = c.ss_part; args.eps = c.eps;
    if (s.in_fx) args.rs_ss_out = c.fx_ss_out;
    if (c.rsd) { args.rs_slab = c.rsd->slab; args.rs_S = c.rsd->S; args.rs_svh = (const half_t*) c.rsd->svh; args.rs_resid_out = (half_t*) c.rsd->resid_out; args.rs_ss_out = c.rsd->ss_out; }
    if (c.act_rs) args.act_rs = *c.act_rs;
    if (c.attm) { args.attm = *c.attm; args.attm.magic_gq = gemv_magic((uint32_t) c.attm->gq); }
    if (c.qkvm) args.qkvm = *c.qkvm;
    if (c.tbl) args.tbl = *c.tbl;
    const int gcb = p.cpw > 0 ? p.cpw : 1;                   // mat[i].cb_first counts the grid's workgroup columns
    int cbf = 0; int64_t wso = 0;
    for (int i = 0; i < nmat; ++i)
    {
        args.mat[i].B = (const uint32_t*) c.Bs[i];
        args.mat[i].suh = c.suhs ? (const half_t*) c.suhs[i] : nullptr;
        args.mat[i].svh = c.svhs ? (const half_t*) c.svhs[i] : nullptr;
        args.mat[i].bias = c.biases ? (const half_t*) c.biases[i] : nullptr;
        args.mat[i].C = c.Cs ? c.Cs[i] : nullptr;
        args.mat[i].xh = pre_xh[i] ? (const half_t*) pre_xh[i] : (c.xhs ? (const half_t*) c.xhs[i] : nullptr);
        args.mat[i].xsum = c.xsums ? c.xsums[i] : nullptr;
        args.mat[i].n = c.ns[i];
        args.mat[i].cb_first = cbf;
        args.mat[i].ws_offset = (int) wso;
        cbf += (c.ns[i] / 128 + gcb - 1) / gcb;
        wso += (int64_t) (c.ns[i] / 128) * p.S * mp * 128;
    }
    for (int i = 1; i < GEMV_MAX_MATS; ++i) args.cbf[i - 1] = args.mat[i].cb_first;
    if (c.epi)
    {
        args.epi = *c.epi;
        args.epi.tickets = ctx->tickets;
        args.epi.ticket_global = s.total_cb;
        args.epi.ss_offset = (int) wso;
        args.epi.xcd_local = p.xcd_local;
        args.epi.rows_per_pass = p.rows_per_pass;
    }
    float* ws_region = ctx->workspace;
    if ((p.S > 1 || s.deferred) && !s.atomic_out)
    {
        ws_region += ctx->ws_toggle ? EXL3_WS_REGION_BYTES / 4 : 0;
        ctx->ws_toggle ^= 1;
        if (c.slabs_out) for (int i = 0; i < nmat; ++i) c.slabs_out[i] = ws_region + args.mat[i].ws_offset;
        if (c.slabs_out && c.tbl) c.slabs_out[0] = ws_region;                // indexed form: [slot][column block][S][m][128]
    }
    if (c.S_out) *c.S_out = p.S;
    args.flags = s.flags | (p.pre_xh ? GEMV_IN_ROTATED : 0);
    args.A = (const half_t*) c.A + (size_t) m0 * c.k;
    args.workspace = ws_region;
    {
        // diagnostics builds (-DG2_TIMING / -DG4_TIMING): phase stamps at 48 MiB of the workspace; EXL3_HIP_TIMING_SLOTS=n (<= 8) rotates n 512-KB slots
        // over successive launches so that a whole captured step keeps the stamps of its last n GEMV launches (slots 4..7 overlap the
        // pre-rotation region at 50 MiB: diagnostics only)
        static const int slots = [] { const char* e = getenv("EXL3_HIP_TIMING_SLOTS"); const int v = e ? atoi(e) : 1; return v < 1 ? 1 : (v > 8 ? 8 : v); }();
        static unsigned launch_no = 0;
        args.ws_debug = ctx->workspace + (48ll << 20) / 4 + (size_t) (slots > 1 ? (launch_no++ % (unsigned) slots) : 0) * (512ll << 10) / 4;
    }
    args.num_mats = c.tbl ? 1 : c.count;
    args.m = mp;
    args.k = c.k;
    args.S = p.S;
    args.kslice = p.bps * 128;
    args.c_fp32 = c.c_fp32;
    args.c_row_offset = m0;
    args.cpw = c.cpw;
    args.chunk_blocks = p.chunk_blocks;
    args.magic_m = gemv_magic((uint32_t) mp);
    if (p.gen != 3) { args.nwv = p.nwv; args.magic_nwv = gemv_magic((uint32_t) p.nwv); args.magic_nhw = gemv_magic((uint32_t) (2 * p.nwv)); }
    return EXL3_OK;
}

static int gemv_launch(const GemvShape& s, const GemvPlan& p, int var, GemvArgs& args, hipStream_t st)
{
    const dim3 grid((unsigned) p.grid_x, (unsigned) p.grid_y, (unsigned) p.grid_z);
    if (p.gen == 3) g_launch_gen3[s.K - 1](s.cb, p.sel, var, p.nwv, grid, (size_t) p.lds, st, args);
    else (p.gen == 4 ? g_launch_gen4 : g_launch_gen2)[s.K - 1](s.cb, var, p.sel, p.nwv, grid, (size_t) p.lds, st, args);
    int rc = exl3_check_launch("exl3_gemv");
    if (rc || !p.reduce) return rc;
    // the reduce kernel walks COLUMN BLOCKS: a launch whose grid counted groups of column blocks (generation 3 with 8- / 16-wave workgroups, the
    // wave-per-column-block layout) hands it the matrices' first column blocks, not their first groups
    if (!s.tbl) { int cbc = 0; for (int i = 0; i < s.count; ++i) { args.mat[i].cb_first = cbc; cbc += s.ns[i] / 128; } }
    const int64_t items = (int64_t) s.total_cb * p.rows;
    exl3_gemv_reduce_kernel<<<dim3((unsigned) ((items + 7) / 8)), dim3(256), 0, st>>>(args, s.total_cb);
    return exl3_check_launch("exl3_gemv_reduce");
}

// The dispatcher: > 0 on success (entry points that promise EXL3_OK map it), < 0 = error code
static int gemv_run(const GemvCall& c)
{
    const FxZeroReq fxz = take_fx_zero();          // one-shot: whatever happens below, the request does not survive this call
    GemvShape s;
    int rc = gemv_validate(c, fxz.ptr != nullptr, s);
    if (rc) return rc;
    Exl3DevCtx* ctx = exl3_get_ctx(c.stream);
    if (!ctx) return EXL3_ERR_INIT;
    const GemvTuning t = gemv_tuning();
    const int pass_rows = gemv_pass_rows(s, t);
    for (int m0 = 0; m0 < c.m; m0 += pass_rows)
    {
        GemvPlan p; GemvArgs args;
        if ((rc = gemv_plan_pass(s, (c.m - m0) < pass_rows ? (c.m - m0) : pass_rows, ctx->num_cus, t, p))) return rc;
        const void* pre_xh[GEMV_MAX_MATS] = { nullptr };
        const size_t xh_bytes = (size_t) p.rows * c.k * 2;
        for (int i = 0; p.pre_xh && i < c.count; ++i)
        {
            // identical suh -> one rotation serves both (gate / up of some checkpoints share it; cheap pointer test)
            for (int j = 0; j < i && !pre_xh[i]; ++j) if (c.suhs[j] == c.suhs[i]) pre_xh[i] = pre_xh[j];
            if (pre_xh[i]) continue;
            void* dst = (char*) ctx->workspace + EXL3_WS_XH_OFFSET + (size_t) i * xh_bytes;
            if ((rc = exl3_had_r_128((const half_t*) c.A + (size_t) m0 * c.k, dst, c.suhs[i], nullptr, 1.0f, p.rows, c.k, 0, c.stream)) != EXL3_OK) return rc;
            pre_xh[i] = dst;
        }
        if ((rc = gemv_fill_args(c, s, p, m0, ctx, pre_xh, fxz, args))) return rc;
        if ((rc = gemv_launch(s, p, t.variant, args, c.stream))) return rc;
    }
    return 1;
}

// The per-matrix tables of a one-matrix request (C, svh optional: their tables are left out when null)
struct GemvOne { const void* B[1]; void* C[1]; const void* suh[1]; const void* svh[1]; const void* bias[1]; int n[1]; };
static GemvCall gemv_call_one(GemvOne& o, const void* B, void* C, const void* suh, const void* svh, const void* bias, int n, int m, int k, int K, int cb,
                              void* stream)
{
    o.B[0] = B; o.C[0] = C; o.suh[0] = suh; o.svh[0] = svh; o.bias[0] = bias; o.n[0] = n;
    GemvCall c = {};
    c.Bs = o.B; c.Cs = C ? o.C : nullptr; c.suhs = o.suh; c.svhs = svh ? o.svh : nullptr; c.biases = o.bias; c.ns = o.n;
    c.count = 1; c.m = m; c.k = k; c.K = K; c.cb = cb; c.stream = (hipStream_t) stream;
    return c;
}
// A request over `count` matrices given as tables
static GemvCall gemv_call_many(const void* A, const void* const* Bs, const void* const* suhs, const int* ns, int count, int m, int k, int K, int cb, void* stream)
{
    GemvCall c = {};
    c.A = A; c.Bs = Bs; c.suhs = suhs; c.ns = ns; c.count = count; c.m = m; c.k = k; c.K = K; c.cb = cb; c.stream = (hipStream_t) stream;
    return c;
}

extern "C" int exl3_gemm(const void* A, const void* B, void* C, const void* suh, const void* svh, const void* bias,
                         int m, int k, int n, int K, int cb, int c_fp32, int force_split, void* stream)
{
    GemvOne o;
    GemvCall c = gemv_call_one(o, B, C, suh, svh, bias, n, m, k, K, cb, stream);
    c.A = A; c.c_fp32 = c_fp32; c.force_split = force_split;
    return gemv_run(c);
}

extern "C" int exl3_mgemm(const void* A, const void* const* Bs, void* const* Cs, const void* const* suhs, const void* const* svhs,
                          const int* ns, int count, int m, int k, int K, int cb, int c_fp32, int force_split, void* stream)
{
    EXL3_CHECK_ARG(Bs && Cs && suhs && svhs && ns, "exl3_mgemm: null table");
    GemvCall c = gemv_call_many(A, Bs, suhs, ns, count, m, k, K, cb, stream);
    c.Cs = Cs; c.svhs = svhs; c.c_fp32 = c_fp32; c.force_split = force_split;
    return gemv_run(c);
}

// Extended launch used by the fused decode pipeline (exl3_glue.hip): optional pre-rotated inputs per matrix and/or deferred
// epilogue (raw fp32 partial slabs left in the per-device workspace for a glue kernel).  slabs_out[i] receives the device
// pointer of matrix i's slabs [n_i/128][S][m][128]; *S_out the split count.
extern "C" int exl3_gemv_ex(const void* A, const void* const* xhs, const float* const* xsums, const void* const* Bs, void* const* Cs,
                            const void* const* suhs, const void* const* svhs, const void* const* biases, const int* ns, int count,
                            int m, int k, int K, int cb, int c_fp32, int flags, int force_split, float** slabs_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(Bs && ns, "exl3_gemv_ex: null table");
    EXL3_CHECK_ARG(!(flags & GEMV_IN_NORM), "exl3_gemv_ex: use exl3_gemv_ex_norm for GEMV_IN_NORM");
    GemvCall c = gemv_call_many(A, Bs, suhs, ns, count, m, k, K, cb, stream);
    c.Cs = Cs; c.svhs = svhs; c.biases = biases; c.c_fp32 = c_fp32; c.force_split = force_split; c.flags = flags;
    c.xhs = xhs; c.xsums = xsums; c.slabs_out = slabs_out; c.S_out = S_out;
    return gemv_run(c);
}

// exl3_gemv_ex whose input A is the fp16 residual stream: RMSNorm (norm_w, eps; per-block sums of squares ss_part [m][k/128] from
// exl3_glue_resid) is applied while the activation fragments are built.  flags: GEMV_OUT_DEFERRED optional.
extern "C" int exl3_gemv_ex_norm(const void* resid, const void* norm_w, const float* ss_part, float eps, const void* const* Bs, void* const* Cs,
                                 const void* const* suhs, const void* const* svhs, const void* const* biases, const int* ns, int count,
                                 int m, int k, int K, int cb, int c_fp32, int flags, int force_split, float** slabs_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(Bs && ns && resid, "exl3_gemv_ex_norm: null table");
    GemvCall c = gemv_call_many(resid, Bs, suhs, ns, count, m, k, K, cb, stream);
    c.Cs = Cs; c.svhs = svhs; c.biases = biases; c.c_fp32 = c_fp32; c.force_split = force_split; c.flags = (flags & GEMV_OUT_DEFERRED) | GEMV_IN_NORM;
    c.slabs_out = slabs_out; c.S_out = S_out; c.norm_w = norm_w; c.ss_part = ss_part; c.eps = eps;
    return gemv_run(c);
}

// ------------------------------------------------------------------------------------------------
// GEMV launches with an in-kernel tail epilogue (exl3_gemv2_tail.cuh): a whole sublayer boundary of the decode step per launch.
// Inputs are either pre-rotated (xhs / xsums from the producing tail or glue kernel) or raw (A + suhs: the kernel rotates).
// ------------------------------------------------------------------------------------------------
// one matrix, fp32 slabs, the tail epilogue e; input xh (+ xsum) when given, else A
static int gemv_run_tail_one(const GemvEpi& e, const void* A, const void* xh, const float* xsum, const void* B, const void* suh, const void* svh, const void* bias,
                             int m, int k, int n, int K, int cb, int force_split, void* stream)
{
    GemvOne o;
    const void* xhs[1] = { xh }; const float* xss[1] = { xsum };
    GemvCall c = gemv_call_one(o, B, nullptr, suh, svh, bias, n, m, k, K, cb, stream);
    c.A = A; c.c_fp32 = 1; c.force_split = force_split; c.epi = &e;
    if (xh) { c.flags = GEMV_IN_ROTATED; c.xhs = xhs; c.xsums = xss; }
    return gemv_run(c);
}

extern "C" int exl3_gemv_norm(const void* A, const void* xh, const float* xsum, const void* B, const void* suh, const void* svh, const void* bias,
                              int m, int k, int n, int K, int cb, void* resid, const void* norm_w, float eps,
                              const void* const* t_suhs, void* const* t_xhs, float* const* t_xsums, int t_count, void* xn_out, void* stream)
{
    EXL3_CHECK_ARG(B && svh && resid && norm_w, "exl3_gemv_norm: null pointer");
    EXL3_CHECK_ARG(m >= 1 && m <= 16, "exl3_gemv_norm: 1 <= m <= 16");
    EXL3_CHECK_ARG(t_count >= 0 && t_count <= 3, "exl3_gemv_norm: at most 3 consumers");
    GemvEpi e; memset((void*) &e, 0, sizeof(e));
    e.mode = GEMV_EPI_NORM;
    e.resid = (half_t*) resid; e.norm_w = (const half_t*) norm_w; e.eps = eps; e.xn_out = (half_t*) xn_out; e.t_count = t_count;
    for (int i = 0; i < t_count; ++i)
    {
        EXL3_CHECK_ARG(t_suhs && t_xhs && t_suhs[i] && t_xhs[i], "exl3_gemv_norm: null consumer pointer");
        e.t_suh[i] = (const half_t*) t_suhs[i]; e.t_xh[i] = (half_t*) t_xhs[i]; e.t_xsum[i] = t_xsums ? t_xsums[i] : nullptr;
    }
    return gemv_run_tail_one(e, A, xh, xsum, B, suh, svh, bias, m, k, n, K, cb, 0, stream);
}

// o_proj / down_proj with glue_resid inside the launch: resid (fp16, in place) += linear(x), ss_out[m][n/128] = per-block sums of squares of the
// new residual (what the consumer's GEMV_IN_NORM needs).  The workgroup that finishes a column block last does it; with n/128 % 8 == 0 all
// slices of a column block are placed on one XCD and the hand-off stays in its L2.
extern "C" int exl3_gemv_resid(const void* A, const void* xh, const float* xsum, const void* B, const void* suh, const void* svh, const void* bias,
                               int m, int k, int n, int K, int cb, void* resid, float* ss_out, int force_split, void* stream)
{
    EXL3_CHECK_ARG(B && svh && resid && ss_out, "exl3_gemv_resid: null pointer");
    EXL3_CHECK_ARG(m >= 1 && m <= 16, "exl3_gemv_resid: 1 <= m <= 16");
    GemvEpi e; memset((void*) &e, 0, sizeof(e));
    e.mode = GEMV_EPI_RESID;
    e.resid = (half_t*) resid; e.ss_out = ss_out;
    return gemv_run_tail_one(e, A, xh, xsum, B, suh, svh, bias, m, k, n, K, cb, force_split, stream);
}

extern "C" int exl3_gemv_act(const void* A, const void* const* xhs, const float* const* xsums, const void* const* Bs, const void* const* suhs,
                             const void* const* svhs, int m, int k, int inter, int K, int cb,
                             const void* suh_d, void* xh_d, float* xsum_d, void* a_out, void* stream)
{
    EXL3_CHECK_ARG(Bs && svhs && svhs[0] && svhs[1] && suh_d && xh_d, "exl3_gemv_act: null pointer");
    EXL3_CHECK_ARG(m >= 1 && m <= 16, "exl3_gemv_act: 1 <= m <= 16");
    GemvEpi e; memset((void*) &e, 0, sizeof(e));
    e.mode = GEMV_EPI_ACT;
    e.t_count = 1; e.t_suh[0] = (const half_t*) suh_d; e.t_xh[0] = (half_t*) xh_d; e.t_xsum[0] = xsum_d; e.a_out = (half_t*) a_out;
    int ns[2] = { inter, inter };
    GemvCall c = gemv_call_many(A, Bs, suhs, ns, 2, m, k, K, cb, stream);
    c.svhs = svhs; c.flags = xhs ? GEMV_IN_ROTATED : 0; c.xhs = xhs; c.xsums = xsums; c.epi = &e;
    return gemv_run(c);
}

extern "C" int exl3_gemv_qkv(const void* A, const void* const* xhs, const float* const* xsums, const void* const* Bs, const void* const* suhs,
                             const void* const* svhs, int m, int k, int K, int cb, void* q_out, void* k_out, void* v_out,
                             const float* rope_sin, const float* rope_cos, const int32_t* positions,
                             void* k_cache, void* k_scales, void* v_cache, void* v_scales, const int32_t* block_table, int blocks_per_seq,
                             int page_size, int k_bits, int v_bits, int heads_q, int heads_kv, int head_dim, int rope_mode, void* stream)
{
    EXL3_CHECK_ARG(Bs && svhs && svhs[0] && svhs[1] && svhs[2] && q_out && rope_sin && rope_cos && positions, "exl3_gemv_qkv: null pointer");
    EXL3_CHECK_ARG(head_dim == 128, "exl3_gemv_qkv: head_dim must be 128 (one Hadamard block per head)");
    EXL3_CHECK_ARG(m >= 1 && m <= 16, "exl3_gemv_qkv: 1 <= m <= 16");
    EXL3_CHECK_ARG(rope_mode == 1 || rope_mode == 2, "exl3_gemv_qkv: rope_mode must be 1 (GPTJ) or 2 (NEOX)");
    EXL3_CHECK_ARG(!k_cache || (k_scales && v_cache && v_scales && block_table && page_size > 0), "exl3_gemv_qkv: incomplete cache arguments");
    EXL3_CHECK_ARG(!k_cache || (k_bits >= 2 && k_bits <= 8 && v_bits >= 2 && v_bits <= 8), "exl3_gemv_qkv: cache bits must be in [2, 8]");
    GemvEpi e; memset((void*) &e, 0, sizeof(e));
    e.mode = GEMV_EPI_QKV;
    e.q_out = (half_t*) q_out; e.k_out = (half_t*) k_out; e.v_out = (half_t*) v_out;
    e.rope_sin = rope_sin; e.rope_cos = rope_cos; e.positions = positions;
    e.k_cache = (uint32_t*) k_cache; e.k_scales = (half_t*) k_scales; e.v_cache = (uint32_t*) v_cache; e.v_scales = (half_t*) v_scales;
    e.block_table = block_table; e.blocks_per_seq = blocks_per_seq; e.page_size = page_size > 0 ? page_size : 256;
    e.k_bits = k_bits; e.v_bits = v_bits; e.hq = heads_q; e.hkv = heads_kv; e.rope_mode = rope_mode;
    int ns[3] = { heads_q * 128, heads_kv * 128, heads_kv * 128 };
    GemvCall c = gemv_call_many(A, Bs, suhs, ns, 3, m, k, K, cb, stream);
    c.svhs = svhs; c.flags = xhs ? GEMV_IN_ROTATED : 0; c.xhs = xhs; c.xsums = xsums; c.epi = &e;
    return gemv_run(c);
}

// Indexed / weighted multi-matrix launch (MoE): exl3_mgemm with pointer tables (quant/exl3_gemm.cuh:58-78, kernel exl3_gemm_kernel.cuh:88-292).
//   slot j of bszm: matrix = indices ? indices[j] : j (device int64); with an expert range, in-range entries are compacted to the front and
//   re-based to min_index, the remaining slots are skipped; A [bszm_in][m][k] (bszm_in == 1: shared), C [bszm][m][n];
//   weights (fp16 [bszm]): each slot's output is scaled by its weight inside the output Hadamard scale, then every group of
//   bszm / num_tokens slots is summed into C[t].
// The table block of the indexed entries: slot outputs [m][n] apart, slot inputs [m][k] apart or one shared input, no expert range unless set after
static GemvTable gemv_table(const void* tbl_B, const void* tbl_suh, const void* tbl_svh, const int64_t* indices, const void* weights, void* C, int bszm,
                            int m, int k, int n, bool shared_in)
{
    GemvTable t; memset((void*) &t, 0, sizeof(t));
    t.B = (const uint64_t*) tbl_B; t.suh = (const uint64_t*) tbl_suh; t.svh = (const uint64_t*) tbl_svh;
    t.indices = indices; t.weights = (const half_t*) weights; t.C = C;
    t.bszm = bszm; t.min_index = -1; t.max_index = -1; t.n = n; t.cbs_per_mat = n / 128;
    t.a_slot_stride = shared_in ? 0 : (int64_t) m * k;
    t.c_slot_stride = (int64_t) m * n;
    return t;
}
// A table request: `bszm` slots of one width n (the per-matrix tables stay empty: the kernels read the device-side tables of t)
static GemvCall gemv_call_table(const GemvTable& t, const int* n, const void* A, int m, int k, int K, int cb, void* stream)
{
    GemvCall c = {};
    c.A = A; c.tbl = &t; c.ns = n; c.count = t.bszm; c.m = m; c.k = k; c.K = K; c.cb = cb; c.stream = (hipStream_t) stream;
    return c;
}

static int mgemm_indexed_impl(const void* A, const void* act_u, int bszm_in, const void* tbl_B, const void* tbl_suh, const void* tbl_svh,
                              const int64_t* indices, const void* weights, int bszm, void* C, int m, int k, int n, int K, int cb, int c_fp32,
                              int min_index, int max_index, int num_tokens, void* stream);

extern "C" int exl3_mgemm_indexed(const void* A, int bszm_in, const void* tbl_B, const void* tbl_suh, const void* tbl_svh,
                                  const int64_t* indices, const void* weights, int bszm, void* C, int m, int k, int n, int K, int cb, int c_fp32,
                                  int min_index, int max_index, int num_tokens, void* stream)
{
    return mgemm_indexed_impl(A, nullptr, bszm_in, tbl_B, tbl_suh, tbl_svh, indices, weights, bszm, C, m, k, n, K, cb, c_fp32, min_index, max_index,
                              num_tokens, stream);
}

// exl3_mgemm with per-matrix output widths (quant/exl3_gemm.cuh:54-55, exl3_gemm.cu:433-447, kernel exl3_gemm_kernel.cuh:176-182): matrix i is
// size_n_list[i] columns wide (device int32, multiples of 128, <= n_max) and its [m][size_n_list[i]] output goes to c_ptrs[i] (device int64 table);
// slot j runs matrix indices ? indices[j] : j.  As in the reference: no routing weights, no expert range, one token.
extern "C" int exl3_mgemm_indexed_nlist(const void* A, int bszm_in, const void* tbl_B, const void* tbl_suh, const void* tbl_svh, const int64_t* indices,
                                        int bszm, const int32_t* size_n_list, const void* c_ptrs, int m, int k, int n_max, int K, int cb, int c_fp32,
                                        void* stream)
{
    EXL3_CHECK_ARG(A && tbl_B && tbl_suh && tbl_svh && size_n_list && c_ptrs, "exl3_mgemm (per-matrix widths): null pointer");
    EXL3_CHECK_ARG(bszm >= 1 && (bszm_in == 1 || bszm_in == bszm), "exl3_mgemm: A must have 1 or bszm slots");
    EXL3_CHECK_ARG(m >= 1 && m <= 16, "exl3_mgemm (per-matrix widths): 1..16 rows per slot");
    // (C is never written: every slot's output pointer comes from c_list)
    GemvTable t = gemv_table(tbl_B, tbl_suh, tbl_svh, indices, nullptr, (void*) c_ptrs, bszm, m, k, n_max, bszm_in == 1);
    t.c_slot_stride = 0;
    t.n_list = size_n_list; t.c_list = (const uint64_t*) c_ptrs;
    GemvCall c = gemv_call_table(t, &n_max, A, m, k, K, cb, stream);
    c.c_fp32 = c_fp32;
    return gemv_run(c);
}

// exl3_mgemm_indexed whose input is fp16(silu(G_j) * U_j) per slot (G, U: [bszm][m][k] fp16, the gate / up outputs of the routed experts): the
// silu_mul launch between the gate|up and the down exl3_mgemm of a MoE block (block_sparse_mlp.py / activation.cu) folded into the down launch.
extern "C" int exl3_mgemm_indexed_act(const void* G, const void* U, const void* tbl_B, const void* tbl_suh, const void* tbl_svh,
                                      const int64_t* indices, const void* weights, int bszm, void* C, int m, int k, int n, int K, int cb, int c_fp32,
                                      int min_index, int max_index, int num_tokens, void* stream)
{
    EXL3_CHECK_ARG(U, "exl3_mgemm_indexed_act: null up tensor");
    return mgemm_indexed_impl(G, U, bszm, tbl_B, tbl_suh, tbl_svh, indices, weights, bszm, C, m, k, n, K, cb, c_fp32, min_index, max_index,
                              num_tokens, stream);
}

static int mgemm_indexed_impl(const void* A, const void* act_u, int bszm_in, const void* tbl_B, const void* tbl_suh, const void* tbl_svh,
                              const int64_t* indices, const void* weights, int bszm, void* C, int m, int k, int n, int K, int cb, int c_fp32,
                              int min_index, int max_index, int num_tokens, void* stream)
{
    EXL3_CHECK_ARG(A && tbl_B && tbl_suh && tbl_svh && C, "exl3_mgemm: null pointer");
    EXL3_CHECK_ARG(bszm >= 1 && (bszm_in == 1 || bszm_in == bszm), "exl3_mgemm: A must have 1 or bszm slots");
    EXL3_CHECK_ARG(num_tokens >= 1 && bszm % num_tokens == 0, "exl3_mgemm: bszm must be divisible by num_tokens");
    EXL3_CHECK_ARG(num_tokens == 1 || min_index < 0, "exl3_mgemm: multi-token reduction (num_tokens > 1) is not compatible with expert-range filtering (min_index >= 0); TP-sharded experts must use num_tokens == 1");
    EXL3_CHECK_ARG(min_index < 0 || indices, "exl3_mgemm: an expert range needs indices");
    GemvTable t = gemv_table(tbl_B, tbl_suh, tbl_svh, indices, weights, C, bszm, m, k, n, bszm_in == 1);
    t.min_index = min_index; t.max_index = max_index; t.act_u = (const half_t*) act_u;
    GemvCall c = gemv_call_table(t, &n, A, m, k, K, cb, stream);
    c.c_fp32 = c_fp32;
    int rc = gemv_run(c);
    if (rc < 0) return rc;
    if (weights)
    {
        const int64_t mn = (int64_t) m * n;
        mgemm_slot_reduce_kernel<<<dim3((unsigned) ((mn + 255) / 256)), dim3(256), 0, (hipStream_t) stream>>>(C, c_fp32, num_tokens, bszm / num_tokens, mn, indices, bszm,
                                                                                                               min_index, max_index);
        return exl3_check_launch("exl3_mgemm slot reduce") < 0 ? EXL3_ERR_HIP : rc;
    }
    return rc;
}

// exl3_mgemm_indexed_act with a deferred epilogue: the launch leaves raw rotated-basis split-k slabs [slot][n/128][S][m][128] fp32 (no svh, no
// routing weights, no slot sum); exl3_glue_resid_moe finishes them together with the residual add.  No expert range (one rank holds all experts).
extern "C" int exl3_mgemm_indexed_act_deferred(const void* G, const void* U, const void* tbl_B, const void* tbl_suh, const int64_t* indices, int bszm,
                                               int m, int k, int n, int K, int cb, float** slab_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(G && U && tbl_B && tbl_suh && indices && slab_out && S_out, "exl3_mgemm_indexed_act_deferred: null pointer");
    EXL3_CHECK_ARG(bszm >= 1 && m >= 1 && m <= 4, "exl3_mgemm_indexed_act_deferred: 1..4 rows per slot");
    GemvTable t = gemv_table(tbl_B, tbl_suh, nullptr, indices, nullptr, nullptr, bszm, m, k, n, false);
    t.act_u = (const half_t*) U;
    GemvCall c = gemv_call_table(t, &n, G, m, k, K, cb, stream);
    c.flags = GEMV_OUT_DEFERRED; c.slabs_out = slab_out; c.S_out = S_out;
    const int rc = gemv_run(c);
    return rc < 0 ? rc : EXL3_OK;
}

// Indexed gate|up launch of a MoE block with a deferred epilogue (generation 4): raw x (bszm_in == 1: one shared row set), pointer tables over
// [gate_0..gate_E-1, up_0..up_E-1], indices = the router's [gate slots | up slots] list; leaves slabs [slot][n/128][S][m][128] for
// exl3_mgemm_indexed_act_fx.
extern "C" int exl3_mgemm_indexed_deferred(const void* A, int bszm_in, const void* tbl_B, const void* tbl_suh, const int64_t* indices, int bszm,
                                           int m, int k, int n, int K, int cb, int force_split, float** slab_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(A && tbl_B && tbl_suh && slab_out && S_out, "exl3_mgemm_indexed_deferred: null pointer");
    EXL3_CHECK_ARG(bszm >= 1 && (bszm_in == 1 || bszm_in == bszm) && m >= 1 && m <= 4, "exl3_mgemm_indexed_deferred: 1..4 rows per slot; A has 1 or bszm slots");
    const GemvTable t = gemv_table(tbl_B, tbl_suh, nullptr, indices, nullptr, nullptr, bszm, m, k, n, bszm_in == 1);
    GemvCall c = gemv_call_table(t, &n, A, m, k, K, cb, stream);
    c.force_split = force_split; c.flags = GEMV_OUT_DEFERRED; c.slabs_out = slab_out; c.S_out = S_out;
    const int rc = gemv_run(c);
    return rc < 0 ? rc : EXL3_OK;
}

// Indexed down launch of a MoE block in the fx pipeline (generation 4): slot j's input is fp16(silu(g_j) * u_j) finished from the slabs of
// exl3_mgemm_indexed_deferred (gate slots first, then the up slots: gu_slabs, act_S; gu_svh_tbl = that launch's svh table, up svh = entry + up_off),
// its output rows -- out-Hadamard, svh and the routing weight applied per split-k partial -- are ADDED into the fixed-point residual accumulator
// R [num_tokens][m][n] int64 (slot j -> token j / (bszm / num_tokens)): no slot sum, no split-k reduce, no residual launch.
extern "C" int exl3_mgemm_indexed_act_fx(const float* gu_slabs, int act_S, const void* gu_svh_tbl, int up_off, const void* tbl_B, const void* tbl_suh,
                                         const void* tbl_svh, const int64_t* indices, const void* weights, int bszm, void* R, int m, int k, int n,
                                         int K, int cb, int num_tokens, int force_split, void* stream)
{
    EXL3_CHECK_ARG(gu_slabs && gu_svh_tbl && tbl_B && tbl_suh && tbl_svh && R, "exl3_mgemm_indexed_act_fx: null pointer");
    EXL3_CHECK_ARG(bszm >= 1 && m >= 1 && m <= 4 && act_S >= 1, "exl3_mgemm_indexed_act_fx: 1..4 rows per slot");
    EXL3_CHECK_ARG(num_tokens >= 1 && bszm % num_tokens == 0, "exl3_mgemm_indexed_act_fx: bszm must be divisible by num_tokens");
    GemvTable t = gemv_table(tbl_B, tbl_suh, tbl_svh, indices, weights, R, bszm, m, k, n, true);
    t.act_svh = (const uint64_t*) gu_svh_tbl; t.act_up_off = up_off; t.slots_per_token = bszm / num_tokens;
    GemvCall c = gemv_call_table(t, &n, nullptr, m, k, K, cb, stream);
    c.force_split = force_split; c.flags = GEMV_OUT_ATOMIC;
    c.act_g = gu_slabs; c.act_u = gu_slabs + (size_t) bszm * ((size_t) (k / 128) * act_S * m * 128); c.act_S = act_S;
    const int rc = gemv_run(c);
    return rc < 0 ? rc : EXL3_OK;
}

// down_proj whose input a = fp16(silu(g) * u) is finished from the gate / up launch's deferred slabs while the activation fragments are
// built (m <= 4): replaces exl3_glue_act + exl3_gemv_ex(IN_ROTATED).  g_slabs / u_slabs / act_S: as returned by the gate / up exl3_gemv_ex
// call (they live in the other workspace region than this launch's own slabs).  flags: EXL3_GEMV_OUT_DEFERRED optional.
// exl3_gemv_ex_norm that also finishes the PRODUCER linear's residual add (replaces the exl3_glue_resid launch between o_proj / down_proj and the
// next q|k|v / gate|up launch at m <= 4).  resid_in: fp16 [m][k] residual BEFORE the producer's output is added (read only); prod_slabs / prod_S /
// prod_svh: the producer's deferred slabs (exl3_gemv_ex*, GEMV_OUT_DEFERRED; they live in the other workspace region); every workgroup rebuilds
// resid_new = resid_in + linear_out for the Hadamard blocks of its k-slice, the column-block-0 workgroups write resid_out (a different buffer)
// and ss_out [m][k/128].  The RMSNorm row scale comes from ss_prev (sums of squares of resid_in): consumers of THIS launch's deferred slabs apply
// rsqrt(mean(resid_new^2) + eps) / rsqrt(mean(resid_in^2) + eps) (exl3_glue_qkv_rs, exl3_gemv_ex_act_rs).  Output: always deferred slabs.
extern "C" int exl3_gemv_ex_resid(const void* resid_in, const void* norm_w, const float* ss_prev, float eps, const float* prod_slabs, int prod_S,
                                  const void* prod_svh, void* resid_out, float* ss_out, const void* const* Bs, const void* const* suhs, const int* ns,
                                  int count, int m, int k, int K, int cb, int cpw, int force_split, float** slabs_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(Bs && ns && resid_in && suhs, "exl3_gemv_ex_resid: null table");
    const GemvResidIn rsd = { prod_slabs, prod_S, prod_svh, resid_out, ss_out };
    GemvCall c = gemv_call_many(resid_in, Bs, suhs, ns, count, m, k, K, cb, stream);
    c.force_split = force_split; c.flags = GEMV_OUT_DEFERRED | GEMV_IN_NORM; c.slabs_out = slabs_out; c.S_out = S_out;
    c.norm_w = norm_w; c.ss_part = ss_prev; c.eps = eps; c.rsd = &rsd; c.cpw = cpw > 0 ? cpw : 4;
    return gemv_run(c);
}

// The "fx" decode pipeline (round 3): the residual stream lives in a 64-bit fixed-point accumulator R [m][hidden] (value * 2^32).  o_proj / down_proj
// launches ADD their output rows into it (exl3_gemv_ex with EXL3_GEMV_OUT_ATOMIC: integer atomics, order-independent, so no split-k reduce and no
// residual launch), and this launch is the consumer: exl3_gemv_ex_norm whose input is R.  The RMSNorm scale it applies is the PREVIOUS residual's
// (ss_prev [m][k/128], complete) because the sums of squares of R itself are only known once every block has been read: the workgroups of column
// block 0 write them to ss_out, and whoever finishes this launch's slabs multiplies by r_new / r_prev (exl3_glue_qkv_rs, exl3_glue_act_rs) -- the
// protocol of exl3_gemv_ex_resid without its redundant slab reduction (the memory system has already summed the slices).  Output: deferred slabs.
extern "C" int exl3_gemv_ex_fx(const void* R, const void* norm_w, const float* ss_prev, float* ss_out, float eps, const void* const* Bs,
                               const void* const* suhs, const int* ns, int count, int m, int k, int K, int cb, int force_split,
                               float** slabs_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(Bs && ns && R && suhs && ss_prev && ss_out && ss_prev != ss_out, "exl3_gemv_ex_fx: null table / ss_out must differ from ss_prev");
    GemvCall c = gemv_call_many(R, Bs, suhs, ns, count, m, k, K, cb, stream);
    c.force_split = force_split; c.flags = GEMV_OUT_DEFERRED | GEMV_IN_NORM | GEMV_IN_FX; c.slabs_out = slabs_out; c.S_out = S_out;
    c.norm_w = norm_w; c.ss_part = ss_prev; c.eps = eps; c.fx_ss_out = ss_out;
    return gemv_run(c);
}

// exl3_gemv_ex_fx whose outputs are ADDED into fixed-point accumulators accs[i] (int64 [m][n_i], zero on entry: exl3_fx_zero_next) instead of being
// left as slabs: gate|up of the fx pipeline.  The rows still carry the previous residual's 1/rms: the consumer (exl3_gemv_ex_actfx) corrects.
extern "C" int exl3_gemv_ex_fx_atomic(const void* R, const void* norm_w, const float* ss_prev, float* ss_out, float eps, const void* const* Bs,
                                      void* const* accs, const void* const* suhs, const void* const* svhs, const int* ns, int count, int m, int k, int K,
                                      int cb, int force_split, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(Bs && ns && R && suhs && svhs && accs && ss_prev && ss_out && ss_prev != ss_out, "exl3_gemv_ex_fx_atomic: null table");
    GemvCall c = gemv_call_many(R, Bs, suhs, ns, count, m, k, K, cb, stream);
    c.Cs = accs; c.svhs = svhs; c.force_split = force_split; c.flags = GEMV_OUT_ATOMIC | GEMV_IN_NORM | GEMV_IN_FX; c.S_out = S_out;
    c.norm_w = norm_w; c.ss_part = ss_prev; c.eps = eps; c.fx_ss_out = ss_out;
    return gemv_run(c);
}

// The one-matrix launches whose input is finished inside the launch (ACT / ACTFX / ATTM / QKVM): output final (C, svh, bias), deferred slabs or atomic
static GemvCall gemv_call_one_ex(GemvOne& o, const void* B, void* C, const void* suh, const void* svh, const void* bias, int n, int m, int k, int K, int cb,
                                 int c_fp32, int flags, int force_split, float** slab_out, int* S_out, void* stream)
{
    GemvCall c = gemv_call_one(o, B, C, suh, svh, bias, n, m, k, K, cb, stream);
    c.c_fp32 = c_fp32; c.flags = flags & (GEMV_OUT_DEFERRED | GEMV_OUT_ATOMIC); c.force_split = force_split; c.slabs_out = slab_out; c.S_out = S_out;
    return c;
}

// down_proj of the fx pipeline: input = fp16(silu(g) * u) formed from the fixed-point gate / up accumulators (int64 [m][k]) with the row-scale
// correction r_new / r_prev (ss_prev / ss_new [m][hidden/128]); output added into the residual accumulator R (EXL3_GEMV_OUT_ATOMIC) or left as slabs.
extern "C" int exl3_gemv_ex_actfx(const void* g_acc, const void* u_acc, const float* ss_prev, const float* ss_new, int hidden, float eps,
                                  const void* B, void* C, const void* suh, const void* svh, const void* bias, int m, int k, int n, int K, int cb,
                                  int flags, int force_split, float** slab_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(g_acc && u_acc && B && suh && m <= 4, "exl3_gemv_ex_actfx: null pointer / m <= 4");
    GemvOne o;
    const GemvRescale rs = { ss_prev, ss_new, hidden, eps };
    GemvCall c = gemv_call_one_ex(o, B, C, suh, svh, bias, n, m, k, K, cb, 0, flags, force_split, slab_out, S_out, stream);
    // the accumulators travel in the act_g / act_u fields; act_S = 1 and dummy svh pointers satisfy the slab-mode argument checks
    c.flags |= GEMV_IN_ACTFX; c.act_g = (const float*) g_acc; c.act_u = (const float*) u_acc; c.act_S = 1; c.act_svh_g = suh; c.act_svh_u = suh;
    if (ss_prev && ss_new) c.act_rs = &rs;
    return gemv_run(c);
}

// exl3_gemv_ex (raw input A + suhs, deferred output, m <= 4) in the wave-per-column-block layout: cpw column blocks of one matrix per workgroup,
// every wave streams the whole k-slice of its column block and writes its own slab (no cross-wave reduction).  cpw in [1, 16].
extern "C" int exl3_gemv_ex_wpc(const void* A, const void* const* Bs, const void* const* suhs, const int* ns, int count, int m, int k, int K, int cb,
                                int cpw, int force_split, float** slabs_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(Bs && ns && A && suhs && cpw >= 1, "exl3_gemv_ex_wpc: null table / cpw");
    GemvCall c = gemv_call_many(A, Bs, suhs, ns, count, m, k, K, cb, stream);
    c.force_split = force_split; c.flags = GEMV_OUT_DEFERRED; c.slabs_out = slabs_out; c.S_out = S_out; c.cpw = cpw;
    return gemv_run(c);
}

// exl3_gemv_ex_act whose gate / up slabs come from an exl3_gemv_ex_resid launch: g and u are multiplied by the exact-over-estimated RMSNorm
// scale of their row (ss_prev / ss_new [m][hidden/128], eps) before svh and silu.
extern "C" int exl3_gemv_ex_act_rs(const float* g_slabs, const float* u_slabs, int act_S, const void* svh_g, const void* svh_u,
                                   const float* ss_prev, const float* ss_new, int hidden, float eps,
                                   const void* B, void* C, const void* suh, const void* svh, const void* bias, int m, int k, int n, int K, int cb,
                                   int c_fp32, int flags, int cpw, int force_split, float** slab_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(B && suh && ss_prev && ss_new && hidden % 128 == 0, "exl3_gemv_ex_act_rs: null pointer");
    GemvOne o;
    const GemvRescale rs = { ss_prev, ss_new, hidden, eps };
    GemvCall c = gemv_call_one_ex(o, B, C, suh, svh, bias, n, m, k, K, cb, c_fp32, flags, force_split, slab_out, S_out, stream);
    c.act_g = g_slabs; c.act_u = u_slabs; c.act_S = act_S; c.act_svh_g = svh_g; c.act_svh_u = svh_u; c.act_rs = &rs; c.cpw = cpw;
    return gemv_run(c);
}

// o_proj whose input is the decode attention's output, finished inside the launch: `part` = the context-split partial records exl3_attn_decode_qcache_split
// left ([m][blocks][gq][nsplit][132] fp32), merged per (row, query head) by the preparation task that needs that head (head_dim 128: one head = one
// Hadamard block of o_proj's input) with the arithmetic of the merge kernel -- same bits as attn_decode_qcache + exl3_gemv_ex, one launch less.
// flags: GEMV_OUT_DEFERRED or GEMV_OUT_ATOMIC (C = the fixed-point residual) or 0 (final output).  reference: libtorch/attention.cpp:246-504 (attention, then o_proj).
extern "C" int exl3_gemv_ex_attm(const float* part, int nsplit, int gq, int blocks, int head_dim, const void* B, void* C, const void* suh, const void* svh, const void* bias,
                                 int m, int k, int n, int K, int cb, int c_fp32, int flags, int force_split, float** slab_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(part && B && suh, "exl3_gemv_ex_attm: null pointer");
    GemvOne o;
    const GemvAttm at = { part, nsplit, gq, blocks, 0u, head_dim };
    GemvCall c = gemv_call_one_ex(o, B, C, suh, svh, bias, n, m, k, K, cb, c_fp32, flags, force_split, slab_out, S_out, stream);
    c.attm = &at;
    return gemv_run(c);
}

// o_proj fed straight by the q|k|v launch's deferred slabs (the decode step WITHOUT the attention core: o_proj's input is the finished q): the q|k|v epilogue
// -- exl3_glue_qkv_tab's work: split-k reduce, output Hadamard, row-scale correction, svh, RoPE from the per-step tables, the 4-bit append of K / V --
// runs inside this launch: a preparation task finishes the q block it needs, idle half-waves of the column-block-0 workgroups append K / V.  Same bits
// as exl3_glue_qkv_tab + exl3_gemv_ex (shared device functions); one launch less per layer.  head_dim 64 | 128, 4-bit K and V.
// reference: libtorch/attention.cpp:283-400 (q / k / v epilogues, rope, cache append) + :497-508 (o_proj).
extern "C" int exl3_gemv_ex_qkvm(const float* sq, const float* sk, const float* sv, int S_qkv, const void* svh_q, const void* svh_k, const void* svh_v,
                                 const float* rope_sin, const float* rope_cos, const int64_t* slots, const float* ss_prev, const float* ss_new, int hidden, float eps,
                                 int rope_mode, int head_dim, int heads_kv, void* q_out, void* k_cache, void* k_scales, void* v_cache, void* v_scales,
                                 const void* B, void* C, const void* suh, const void* svh, const void* bias, int m, int k, int n, int K, int cb, int c_fp32,
                                 int flags, int force_split, float** slab_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(B && suh, "exl3_gemv_ex_qkvm: null pointer");
    EXL3_CHECK_ARG(!ss_new || (ss_prev && hidden > 0 && hidden % 128 == 0), "exl3_gemv_ex_qkvm: rescale needs ss_prev and hidden");
    EXL3_CHECK_ARG((head_dim == 64 || head_dim == 128) && heads_kv >= 1 && (heads_kv * head_dim) % 128 == 0, "exl3_gemv_ex_qkvm: head_dim 64 | 128, whole 128-value kv blocks");
    GemvQkvm q; memset((void*) &q, 0, sizeof(q));
    q.sq = sq; q.sk = sk; q.sv = sv; q.S = S_qkv; q.rope_mode = rope_mode;
    q.svh_q = (const half_t*) svh_q; q.svh_k = (const half_t*) svh_k; q.svh_v = (const half_t*) svh_v;
    q.rope_sin = rope_sin; q.rope_cos = rope_cos; q.slots = slots;
    q.rs = GemvRescale{ ss_prev, ss_new, hidden, eps };
    q.q_out = (half_t*) q_out; q.k_cache = (uint32_t*) k_cache; q.k_scales = (half_t*) k_scales; q.v_cache = (uint32_t*) v_cache; q.v_scales = (half_t*) v_scales;
    q.hd = head_dim; q.kvb = heads_kv * head_dim / 128;
    GemvOne o;
    GemvCall c = gemv_call_one_ex(o, B, C, suh, svh, bias, n, m, k, K, cb, c_fp32, flags, force_split, slab_out, S_out, stream);
    c.qkvm = &q;
    return gemv_run(c);
}

extern "C" int exl3_gemv_ex_act(const float* g_slabs, const float* u_slabs, int act_S, const void* svh_g, const void* svh_u,
                                const void* B, void* C, const void* suh, const void* svh, const void* bias, int m, int k, int n, int K, int cb,
                                int c_fp32, int flags, int force_split, float** slab_out, int* S_out, void* stream)
{
    EXL3_CHECK_ARG(B && suh, "exl3_gemv_ex_act: null pointer");
    GemvOne o;
    GemvCall c = gemv_call_one_ex(o, B, C, suh, svh, bias, n, m, k, K, cb, c_fp32, flags, force_split, slab_out, S_out, stream);
    c.act_g = g_slabs; c.act_u = u_slabs; c.act_S = act_S; c.act_svh_g = svh_g; c.act_svh_u = svh_u;
    return gemv_run(c);
}

// Diagnostics: what the dispatcher launches for a request of this shape on a chip of num_cus CUs, one GemvPlan record per pass -- gemv_validate and
// gemv_plan_pass, the functions gemv_run calls, on a request whose operands are stand-ins: no device, no context, the fx-zero request untouched
// (tests/test_gemv_plan.py replays a recording of the dispatcher's decisions through it).  flags: the GEMV_* bits of exl3_gemv_args.h; operands:
// EXL3_PLAN_* bits (include/exl3_hip.h); attm_hd != 0: a GEMV_IN_ATTM request; tail_xcd_local < 0: the current setting.
extern "C" int exl3_gemv_plan(int flags, const int* ns, int count, int m, int k, int K, int cb, int force_split, int cpw, int operands, int epi_mode,
                              int attm_hd, int attm_nsplit, int num_cus, int tail_xcd_local, int32_t* plans_out, int max_passes, int* passes_out)
{
    EXL3_CHECK_ARG(ns && plans_out && passes_out && max_passes >= 1 && num_cus >= 1, "exl3_gemv_plan: null pointer / sizes");
    static char stand_in[32];
    void* const P = stand_in;
    void* ptrs[GEMV_MAX_MATS] = { P, P, P, P };
    const void* const* cptrs = (const void* const*) ptrs;
    const float* sums[GEMV_MAX_MATS] = { (const float*) P, (const float*) P, (const float*) P, (const float*) P };
    const bool table = (operands & EXL3_PLAN_TABLE) != 0;
    GemvCall c = {};
    c.ns = ns; c.count = count; c.m = m; c.k = k; c.K = K; c.cb = cb; c.force_split = force_split; c.flags = flags; c.cpw = cpw;
    c.A = P;
    if (!table) { c.Bs = cptrs; c.Cs = ptrs; c.suhs = cptrs; c.svhs = cptrs; }
    if (flags & GEMV_IN_ROTATED) c.xhs = cptrs;
    if (operands & EXL3_PLAN_XSUMS) c.xsums = sums;
    if (flags & GEMV_IN_NORM) { c.norm_w = P; c.ss_part = (const float*) P; }
    if ((flags & GEMV_IN_FX) && !(operands & EXL3_PLAN_NO_SS_OUT)) c.fx_ss_out = (float*) P;
    if (operands & EXL3_PLAN_ACT) { c.act_g = c.act_u = (const float*) P; c.act_S = 1; if (!table) c.act_svh_g = c.act_svh_u = P; }
    GemvEpi e; memset((void*) &e, 0, sizeof(e));
    if (epi_mode) { e.mode = epi_mode; c.epi = &e; }
    GemvTable t; memset((void*) &t, 0, sizeof(t));
    if (table)
    {
        t.B = t.suh = t.svh = (const uint64_t*) P; t.C = P; t.slots_per_token = 1;
        if (operands & EXL3_PLAN_TABLE_ACT_U) t.act_u = (const half_t*) P;
        if (operands & EXL3_PLAN_TABLE_N_LIST) t.n_list = (const int32_t*) P;
        if (operands & EXL3_PLAN_ACT) t.act_svh = (const uint64_t*) P;
        c.tbl = &t;
    }
    const GemvAttm at = { (const float*) P, attm_nsplit, 1, k / 128, 0u, attm_hd };
    if (attm_hd) c.attm = &at;
    GemvQkvm q; memset((void*) &q, 0, sizeof(q));
    if (operands & EXL3_PLAN_QKVM)
    {
        q.sq = q.sk = q.sv = q.rope_sin = q.rope_cos = (const float*) P; q.svh_q = q.svh_k = q.svh_v = (const half_t*) P; q.slots = (const int64_t*) P;
        q.k_cache = q.v_cache = (uint32_t*) P; q.k_scales = q.v_scales = (half_t*) P; q.S = 1; q.rope_mode = 1; q.hd = 128; q.kvb = 1;
        c.qkvm = &q;
    }
    const GemvResidIn rsd = { (const float*) P, 1, P, (operands & EXL3_PLAN_RESID_ALIAS) ? P : (void*) (stand_in + 16), (float*) P };
    if (operands & EXL3_PLAN_RESID_IN) c.rsd = &rsd;

    GemvShape s;
    int rc = gemv_validate(c, false, s);
    if (rc) return rc;
    GemvTuning tn = gemv_tuning();
    if (tail_xcd_local >= 0) tn.tail_xcd_local = tail_xcd_local;
    const int pass_rows = gemv_pass_rows(s, tn);
    int passes = 0;
    for (int m0 = 0; m0 < m; m0 += pass_rows, ++passes)
    {
        EXL3_CHECK_ARG(passes < max_passes, "exl3_gemv_plan: more than %d passes", max_passes);
        GemvPlan p;
        if ((rc = gemv_plan_pass(s, (m - m0) < pass_rows ? (m - m0) : pass_rows, num_cus, tn, p))) return rc;
        memcpy(plans_out + passes * EXL3_GEMV_PLAN_INTS, &p, sizeof(p));
    }
    *passes_out = passes;
    return EXL3_OK;
}
