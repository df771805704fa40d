// C-ABI of the trellis encoder (exl3_quantize_tiles.kspec.hip holds the kernel, one unit per K).  Reference: quant/quantize.cu:27-87.
#include "exl3_common.cuh"
#include "exl3_api_internal.h"

#define QT_DECL(KK) \
    void exl3_quantize_tiles_launch_k##KK(const float*, float*, uint16_t*, uint8_t*, int64_t, int64_t, int, hipStream_t); \
    int64_t exl3_quantize_tiles_ws_bytes_k##KK();
QT_DECL(1) QT_DECL(2) QT_DECL(3) QT_DECL(4) QT_DECL(5) QT_DECL(6) QT_DECL(7) QT_DECL(8)
#undef QT_DECL

static int64_t qt_ws_bytes(int K)
{
    switch (K)
    {
        case 1: return exl3_quantize_tiles_ws_bytes_k1();
        case 2: return exl3_quantize_tiles_ws_bytes_k2();
        case 3: return exl3_quantize_tiles_ws_bytes_k3();
        case 4: return exl3_quantize_tiles_ws_bytes_k4();
        case 5: return exl3_quantize_tiles_ws_bytes_k5();
        case 6: return exl3_quantize_tiles_ws_bytes_k6();
        case 7: return exl3_quantize_tiles_ws_bytes_k7();
        default: return exl3_quantize_tiles_ws_bytes_k8();
    }
}

extern "C" int exl3_quantize_tiles_workspace(int K, int64_t* bytes_per_tile)
{
    EXL3_CHECK_ARG(bytes_per_tile, "quantize_tiles_workspace: null pointer");
    EXL3_CHECK_ARG(K >= 1 && K <= 8, "quantize_tiles K must be in range 1..8");
    *bytes_per_tile = qt_ws_bytes(K);
    return EXL3_OK;
}

extern "C" int exl3_quantize_tiles(const void* input, void* output, void* indices, int64_t num_tiles, void* workspace, int64_t max_batch,
                                   int K, int cb, void* stream)
{
    EXL3_CHECK_ARG(K >= 1 && K <= 8, "quantize_tiles K must be in range 1..8");
    EXL3_CHECK_ARG(cb >= 0 && cb <= 2, "quantize_tiles: bad codebook");
    EXL3_CHECK_ARG(num_tiles >= 0, "quantize_tiles: negative tile count");
    if (num_tiles == 0) return EXL3_OK;
    EXL3_CHECK_ARG(input && output && indices && workspace, "quantize_tiles: null pointer");
    EXL3_CHECK_ARG(max_batch >= 1, "quantize_tiles: workspace must hold at least one tile");
    EXL3_CHECK_ARG(max_batch <= 0x7fffffff, "quantize_tiles: batch too large");
    const float* in = (const float*) input;
    float* out = (float*) output;
    uint16_t* idx = (uint16_t*) indices;
    uint8_t* ws = (uint8_t*) workspace;
    hipStream_t st = (hipStream_t) stream;
    switch (K)
    {
        case 1: exl3_quantize_tiles_launch_k1(in, out, idx, ws, num_tiles, max_batch, cb, st); break;
        case 2: exl3_quantize_tiles_launch_k2(in, out, idx, ws, num_tiles, max_batch, cb, st); break;
        case 3: exl3_quantize_tiles_launch_k3(in, out, idx, ws, num_tiles, max_batch, cb, st); break;
        case 4: exl3_quantize_tiles_launch_k4(in, out, idx, ws, num_tiles, max_batch, cb, st); break;
        case 5: exl3_quantize_tiles_launch_k5(in, out, idx, ws, num_tiles, max_batch, cb, st); break;
        case 6: exl3_quantize_tiles_launch_k6(in, out, idx, ws, num_tiles, max_batch, cb, st); break;
        case 7: exl3_quantize_tiles_launch_k7(in, out, idx, ws, num_tiles, max_batch, cb, st); break;
        default: exl3_quantize_tiles_launch_k8(in, out, idx, ws, num_tiles, max_batch, cb, st); break;
    }
    return exl3_check_launch("quantize_tiles");
}
