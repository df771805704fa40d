"""GPU tests of the trellis encoder (exl3_quantize_tiles.kspec.hip, ext.quantize_tiles, exllamav3_amd.quantize): bit-exact against the test-only
restatement of the reference encoder (tests/_trellis_encoder_ref.py) for every K x codebook, batching, properties at a few hundred tiles, and
encode_linear end to end through reconstruct / LinearEXL3 / exl3_gemm."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _trellis_encoder_ref as R                     # noqa: E402
from oracle import exl3_oracle as orc                # noqa: E402

pytestmark = pytest.mark.gpu

CBS = [(0, 1.24371088), (1, 1.24371088), (2, 1.0)]
FLAGS = {0: (False, False), 1: (True, False), 2: (False, True)}
# normalised tile MSE bounds per K: the reference's own (tests/test_quant_fn.py:30-39)
MAX_MSE = {1: 0.3, 2: 0.1, 3: 0.1, 4: 0.1, 5: 0.1, 6: 0.07, 7: 0.05, 8: 0.04}


def _dev():
    return torch.device("cuda:0")


def _ext_quantize(tiles: np.ndarray, K: int, cb: int, batch: int):
    """Through the reference's argument list: temp_costs (b, 2, E) / temp_edges (b, 256, E)."""
    from exllamav3_amd import ext
    dev = _dev()
    x = torch.from_numpy(np.ascontiguousarray(tiles, dtype=np.float32)).to(dev)
    out = torch.zeros_like(x)
    idx = torch.zeros(x.shape, dtype=torch.short, device=dev)
    E = 65536 >> K
    tc = torch.zeros((batch, 2, E), dtype=torch.half, device=dev)
    te = torch.zeros((batch, 256, E), dtype=torch.short, device=dev)
    mcg, mul1 = FLAGS[cb]
    ext.quantize_tiles(x, out, idx, tc, te, K, mcg, mul1)
    torch.cuda.synchronize()
    return out.cpu().numpy(), idx.cpu().numpy().view(np.uint16)


def _exact_inputs(K, cb, scale):
    rng = np.random.default_rng(7 * K + cb)
    x = (rng.standard_normal((3, 256)) * scale).astype(np.float32)
    zero = np.zeros((1, 256), np.float32)
    few = (rng.integers(-2, 3, size=(1, 256)) * 0.5 * scale).astype(np.float32)       # a handful of distinct values: many ties
    return np.concatenate([x, zero, few])


@pytest.mark.parametrize("cb,scale", CBS)
@pytest.mark.parametrize("K", range(1, 9))
def test_quantize_tiles_bit_exact_against_the_restatement(K, cb, scale):
    tiles = _exact_inputs(K, cb, scale)
    out_ref, idx_ref = R.quantize_tiles(tiles, K, cb)
    out, idx = _ext_quantize(tiles, K, cb, batch=8)
    assert np.array_equal(idx, idx_ref), f"K={K} cb={cb}: {np.argwhere(idx != idx_ref)[:8]}"
    assert np.array_equal(out.view(np.uint32), out_ref.view(np.uint32))


@pytest.mark.parametrize("K,cb", [(1, 0), (4, 2), (8, 1)])
def test_quantize_tiles_batching_and_repeatability(K, cb):
    rng = np.random.default_rng(K)
    tiles = (rng.standard_normal((37, 256)) * 1.2).astype(np.float32)
    out1, idx1 = _ext_quantize(tiles, K, cb, batch=64)        # one launch
    out2, idx2 = _ext_quantize(tiles, K, cb, batch=8)         # 5 launches, the last one partial
    out3, idx3 = _ext_quantize(tiles, K, cb, batch=8)
    assert np.array_equal(idx1, idx2) and np.array_equal(out1, out2)
    assert np.array_equal(idx2, idx3) and np.array_equal(out2, out3)
    # n = 0: no launch, nothing written
    from exllamav3_amd import ext
    dev = _dev()
    E = 65536 >> K
    x = torch.zeros((0, 256), device=dev)
    ext.quantize_tiles(x, x.clone(), torch.zeros((0, 256), dtype=torch.short, device=dev),
                       torch.zeros((1, 2, E), dtype=torch.half, device=dev), torch.zeros((1, 256, E), dtype=torch.short, device=dev), K, False, False)


@pytest.mark.parametrize("cb,scale", CBS)
@pytest.mark.parametrize("K", range(1, 9))
def test_quantize_tiles_properties(K, cb, scale):
    from exllamav3_amd import ext, quantize
    dev = _dev()
    rng = np.random.default_rng(1000 + 10 * K + cb)
    n = 300
    x = torch.from_numpy((rng.standard_normal((n, 256)) * scale).astype(np.float32)).to(dev)
    mcg, mul1 = FLAGS[cb]
    out, idx = quantize.quantize_tiles(x, K, mcg, mul1, max_batch=128)
    idx_np = idx.cpu().numpy().view(np.uint16)
    assert R.is_tailbiting(idx_np, K).all()
    dec = torch.empty_like(out)
    ext.decode(idx, dec, mcg, mul1)
    torch.cuda.synchronize()
    assert torch.equal(dec, out)
    mse = ((out - x) / scale).pow(2).mean().item()
    assert mse < MAX_MSE[K], mse
    # ideal inputs (decoded valid tail-biting sequences) come back exactly
    ideal = orc.decode(orc.random_tailbiting_states(rng, (64,), K), cb).astype(np.float32)
    out_i, _ = quantize.quantize_tiles(torch.from_numpy(ideal).to(dev), K, mcg, mul1)
    assert np.array_equal(out_i.cpu().numpy(), ideal)


_ENC_ERR = {}


@pytest.mark.parametrize("cb", [0, 1, 2])
@pytest.mark.parametrize("K", [2, 4, 6])
def test_encode_linear_end_to_end(K, cb):
    from exllamav3_amd import ext, quantize
    from exllamav3_amd.linear import LinearEXL3
    dev = _dev()
    k, n = 256, 512
    mcg, mul1 = FLAGS[cb]
    g = torch.Generator().manual_seed(5)
    w = (torch.randn((k, n), generator=g) * 0.02).to(dev)
    trellis, suh, svh = quantize.encode_linear(w, K, mcg, mul1, seed=3)
    assert trellis.shape == (k // 16, n // 16, 16 * K) and trellis.dtype == torch.short
    assert suh.dtype == torch.half and svh.dtype == torch.half
    # reconstruct(trellis) = the encoder's output tiles placed in (k, n), bit for bit
    tiles, suh2, svh2 = quantize.prepare_tiles(w, K, mcg, mul1, seed=3)
    assert torch.equal(suh, suh2) and torch.equal(svh, svh2)
    out_tiles, _ = quantize.quantize_tiles(tiles, K, mcg, mul1)
    placed = torch.empty_like(out_tiles)
    placed[:, torch.from_numpy(quantize.tensor_core_perm()).to(dev)] = out_tiles
    placed = placed.view(k // 16, n // 16, 16, 16).permute(0, 2, 1, 3).reshape(k, n)
    w_hat = torch.empty((k, n), dtype=torch.half, device=dev)
    ext.reconstruct(w_hat, trellis, K, mcg, mul1)
    torch.cuda.synchronize()
    assert torch.equal(w_hat.float(), placed)
    # relative weight error: bounded by the tile MSE (the rotation is orthonormal, the column scale puts W_hat at the codebook's RMS)
    w_enc = torch.from_numpy(orc.weight_tensor(trellis.cpu().numpy(), suh.cpu().numpy(), svh.cpu().numpy(), K, cb)).to(dev)
    rel = ((w_enc - w).norm() / w.norm()).item()
    bound = 1.5 * MAX_MSE[K] ** 0.5
    assert rel < bound, (rel, bound)
    _ENC_ERR[(K, cb)] = rel
    if all((kk, cb) in _ENC_ERR for kk in (2, 4, 6)):
        assert _ENC_ERR[(2, cb)] > _ENC_ERR[(4, cb)] > _ENC_ERR[(6, cb)], _ENC_ERR
    # the quantized linear: decode GEMV (1 row) and the prefill route (256 rows) give y ~ x @ W
    lin = LinearEXL3(k, n, trellis, suh, svh, mcg=mcg, mul1=mul1)
    for m in (1, 256):
        x = torch.randn((m, k), generator=g).to(dev).half()
        y_ref = x.float() @ w
        y = torch.empty((m, n), dtype=torch.half, device=dev)
        xh = torch.empty_like(x)
        ext.exl3_gemm(x, trellis, y, suh, xh, svh, -1, mcg, mul1, 0)
        torch.cuda.synchronize()
        err = ((y.float() - y_ref).norm() / y_ref.norm()).item()
        assert err < bound, (m, err, bound)
        y2 = lin.forward(x)
        torch.cuda.synchronize()
        err2 = ((y2.float() - y_ref).norm() / y_ref.norm()).item()
        assert err2 < bound, (m, err2, bound)

