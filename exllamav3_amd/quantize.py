"""
The project's own EXL3 encoder entry points, over the gfx950 trellis encoder (exl3_quantize_tiles).

quantize_tiles(tiles, K, mcg, mul1)            -> (out_tiles, idx): tail-biting Viterbi encoding of (n, 256) fp32 tiles in stream order,
                                                   bit-identical to the reference's ext.quantize_tiles (quant/quantize.cu:27-87).
encode_linear(w, K, mcg, mul1, seed)           -> (trellis, suh, svh): a plain encoder of a dense (k, n) weight -- random sign flips, 128-blocked
                                                   Hadamard rotations, a per-column scale folded into svh, no Hessian and no LDLQ (the spirit of
                                                   the reference's fallback_quant, modules/quant/exl3_lib/quantize.py:607-722).  The outputs are
                                                   the tensors LinearEXL3 / ext.exl3_gemm / ext.reconstruct take.

Hessian capture, LDLQ, regularisation and the conversion driver stay the reference's Python, which runs over the stub.
"""
from __future__ import annotations
import ctypes
import math
import numpy as np
import torch

from . import _lib
from . import ext

CODEBOOK_SCALE = 1.24371088          # RMS of the 3INST / mcg codebooks (modules/quant/exl3_lib/quantize.py:16); mul1: 1.0
HAD_DIM = 128

# resident workgroups (tiles) per CU of the encoder kernel by K: K = 1 holds 128 KiB of costs in LDS (one per CU), K = 2..5 run
# 1024-thread workgroups (two fill the CU's 32 wave slots), K = 6 / 7 / 8 run 512 / 256 / 128 threads
_RESIDENT_PER_CU = {1: 1, 2: 2, 3: 2, 4: 2, 5: 2, 6: 4, 7: 8, 8: 16}


def tensor_core_perm() -> np.ndarray:
    """perm[t] = row * 16 + col of stream index t inside a 16x16 tile (modules/quant/exl3_lib/quantize.py:21-44): t = 8 l + j,
    row = 2 (l % 4) + (j & 1) + 8 ((j >> 1) & 1), col = l // 4 + 8 (j >> 2)."""
    t = np.arange(256)
    l, j = t // 8, t % 8
    row = 2 * (l % 4) + (j & 1) + 8 * ((j >> 1) & 1)
    col = l // 4 + 8 * (j >> 2)
    return (row * 16 + col).astype(np.int64)


def _workspace_bytes(K: int) -> int:
    b = ctypes.c_int64(0)
    _lib.check(_lib.lib().exl3_quantize_tiles_workspace(int(K), ctypes.byref(b)))
    return b.value


def batch_tiles(K: int, device: torch.device) -> int:
    """Tiles per launch: two rounds of the resident workgroups of every CU."""
    return 2 * ext.g_get_num_sms(device.index if device.index is not None else torch.cuda.current_device()) * _RESIDENT_PER_CU[int(K)]


def quantize_tiles(tiles: torch.Tensor, K: int, mcg: bool = False, mul1: bool = False, max_batch: int | None = None):
    """tiles: (n, 256) fp32 on a GPU, stream order.  Returns (out_tiles fp32 (n, 256) = decode(idx), idx int16 (n, 256)).
    Allocates only the back-pointer workspace of one batch (exl3_quantize_tiles_workspace(K) bytes per tile)."""
    if not (1 <= int(K) <= 8):
        raise RuntimeError("quantize_tiles K must be in range 1..8")
    if tiles.dim() != 2 or tiles.shape[1] != 256:
        raise RuntimeError("quantize_tiles: tiles must be (n, 256)")
    if tiles.dtype != torch.float:
        raise RuntimeError("quantize_tiles: tiles must be float32")
    if not tiles.is_cuda:
        raise RuntimeError("tensor must be on a GPU device")
    K = int(K)
    tiles = tiles.contiguous()
    n = tiles.shape[0]
    out = torch.empty_like(tiles)
    idx = torch.empty(tiles.shape, dtype=torch.short, device=tiles.device)
    if n == 0:
        return out, idx
    ext._dev(tiles)
    b = min(n, max_batch if max_batch is not None else batch_tiles(K, tiles.device))
    ws = torch.empty(b * _workspace_bytes(K), dtype=torch.uint8, device=tiles.device)
    _lib.check(_lib.lib().exl3_quantize_tiles(tiles.data_ptr(), out.data_ptr(), idx.data_ptr(), n, ws.data_ptr(), b, K,
                                              ext._cb(mcg, mul1), ext._stream(tiles)))
    return out, idx


def _hadamard_128(device) -> torch.Tensor:
    """Orthonormal Sylvester H128 (symmetric, H H = I)."""
    h = torch.ones((1, 1), dtype=torch.float64)
    while h.shape[0] < HAD_DIM:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h / math.sqrt(HAD_DIM)).to(device=device, dtype=torch.float32)


def prepare_tiles(w: torch.Tensor, K: int, mcg: bool = False, mul1: bool = False, seed: int = 0):
    """The rotation half of encode_linear: (tiles fp32 (k/16 * n/16, 256) in stream order, suh fp16 (k), svh fp16 (n)) with
    W = diag(suh) . H . W_hat . H . diag(svh) (128-blocked orthonormal H) and tiles = W_hat cut into 16x16 tiles, row-major over (k/16, n/16)."""
    if w.dim() != 2:
        raise RuntimeError("encode_linear: w must be 2-D (k, n)")
    k, n = w.shape
    if k % HAD_DIM or n % HAD_DIM:
        raise RuntimeError("encode_linear: k and n must be multiples of 128")
    dev = w.device
    scale = 1.0 if (mul1 and not mcg) else CODEBOOK_SCALE
    g = torch.Generator().manual_seed(int(seed))
    su = torch.where(torch.randn(k, generator=g) < 0, -1.0, 1.0)
    sv = torch.where(torch.randn(n, generator=g) < 0, -1.0, 1.0)
    H = _hadamard_128(dev)
    wf = w.to(torch.float32)
    suh = su.to(device=dev, dtype=torch.half)
    # left rotation: A = H . diag(1 / suh) . W  (suh = +-1)
    a = (wf * suh.float()[:, None]).view(k // HAD_DIM, HAD_DIM, n)
    a = torch.matmul(H, a).view(k, n)
    # per-column scale into svh: the columns of A, scaled to the codebook's RMS before the right rotation mixes them
    col_rms = a.pow(2).mean(0).sqrt().clamp_min(1e-8)
    svh = (sv.to(dev) * col_rms / scale).to(torch.half)
    svh = torch.where(svh == 0, torch.full_like(svh, 6e-8), svh)
    a = a / svh.float()[None, :]
    w_hat = torch.matmul(a.view(k, n // HAD_DIM, HAD_DIM), H).view(k, n)
    perm = torch.from_numpy(tensor_core_perm()).to(dev)
    tiles = w_hat.view(k // 16, 16, n // 16, 16).permute(0, 2, 1, 3).reshape(-1, 256)
    tiles = tiles[:, perm].contiguous()
    return tiles, suh, svh


def encode_linear(w: torch.Tensor, K: int, mcg: bool = False, mul1: bool = False, seed: int = 0):
    """Dense (k, n) weight -> (trellis int16 (k/16, n/16, 16K), suh fp16 (k), svh fp16 (n)) with W ~ diag(suh) H reconstruct(trellis) H diag(svh).
    Signs drawn from `seed`; no Hessian, no LDLQ.  k % 128 == 0 and n % 128 == 0."""
    k, n = w.shape
    tiles, suh, svh = prepare_tiles(w, K, mcg, mul1, seed)
    _, idx = quantize_tiles(tiles, K, mcg, mul1)
    trellis = torch.empty((k // 16, n // 16, 16 * int(K)), dtype=torch.short, device=w.device)
    ext.pack_trellis(trellis, idx.view(k // 16, n // 16, 256), int(K))
    return trellis, suh, svh
