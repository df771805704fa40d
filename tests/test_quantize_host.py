"""CPU tests of the trellis encoder feature: the test-only restatement of the reference encoder (tests/_trellis_encoder_ref.py) checked against
itself and a float64 Viterbi, the argmin tie order against a literal restatement of the reference's shuffle-down reduction, the Paley Hadamard
builders, the ext names the reference's converter uses, and argument errors of ext.quantize_tiles without a GPU."""
import ast
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

import _trellis_encoder_ref as R                     # noqa: E402
from oracle import exl3_oracle as orc                # noqa: E402

CBS = [(0, 1.24371088), (1, 1.24371088), (2, 1.0)]
NAMES_RECORD = os.path.join(ROOT, "tests", "golden", "ref_quantizer_ext_names.json")
QUANTIZER_MODULES = ["modules/quant/exl3_lib/quantize.py", "util/hadamard.py"]


@pytest.mark.parametrize("cb,scale", CBS)
@pytest.mark.parametrize("K", range(1, 9))
def test_restated_encoder_self_checks(K, cb, scale):
    rng = np.random.default_rng(100 * K + cb)
    x = (rng.standard_normal((1, 256)) * scale).astype(np.float32)
    ideal = orc.decode(orc.random_tailbiting_states(rng, (1,), K), cb).astype(np.float32)
    tiles = np.concatenate([x, ideal])
    out, idx = R.quantize_tiles(tiles, K, cb)
    assert R.is_tailbiting(idx, K).all()
    assert np.array_equal(out, orc.decode(idx, cb).astype(np.float32))
    # an ideal (decoded, tail-biting) input comes back with zero error (values: two states may decode alike)
    assert np.array_equal(out[1], ideal[0])
    # the path cost is within fp16 accumulation slack of the exact least-cost path through the same start node
    pre = (idx[:, 0].astype(np.int64) >> K)
    w = tiles.astype(np.float16).astype(np.float64)
    path = ((out.astype(np.float64) - w) ** 2).sum(1)
    best = R.viterbi_f64_constrained(tiles, K, cb, pre)
    assert np.all(path >= best - 1e-9)
    assert np.all(path <= best * (1 + 256 * 2.0 ** -11) + 1e-3), (path, best)
    # normalised MSE of the random tile under the reference's per-K bound (tests/test_quant_fn.py:30-39)
    max_mse = {1: 0.3, 2: 0.1, 3: 0.1, 4: 0.1, 5: 0.1, 6: 0.07, 7: 0.05, 8: 0.04}[K]
    assert ((out[0] / scale - x[0] / scale) ** 2).mean() < max_mse


@pytest.mark.parametrize("E", [256, 512, 1024, 2048, 4096, 8192, 16384, 32768])
def test_argmin_tie_order_matches_the_shuffle_down_tree(E):
    rng = np.random.default_rng(E)
    cases = [np.zeros(E), np.full(E, 3.0)]
    cases += [rng.integers(0, m, size=E).astype(np.float64) for m in (2, 3, 5)]
    c = np.ones(E); c[rng.choice(E, 4, replace=False)] = 0.0; cases.append(c)
    c = rng.integers(0, 4, size=E).astype(np.float64); c[:E // 2] = np.inf; cases.append(c)
    for c in cases:
        assert R.argmin_key_order(c) == R.argmin_shuffle_tree(c)


def _paley_sizes(limit=1024):
    def prime(p):
        return p > 1 and all(p % d for d in range(2, int(p ** 0.5) + 1))
    p1 = [n for n in range(4, limit + 1, 4) if prime(n - 1) and (n - 1) % 4 == 3]
    p2 = [n for n in range(4, limit + 1, 4) if prime(n // 2 - 1) and (n // 2 - 1) % 4 == 1]
    p2_any = [n for n in range(4, limit + 1, 4) if prime(n // 2 - 1)]
    return p1, p2, p2_any


def test_had_paley_builds_hadamard_matrices():
    from exllamav3_amd import ext
    p1, p2, _ = _paley_sizes()
    for fn, sizes in ((ext.had_paley, p1), (ext.had_paley2, p2)):
        assert sizes
        for n in sizes:
            h = torch.empty((n, n), dtype=torch.half)
            fn(h)
            hf = h.double()
            assert torch.equal(hf.abs(), torch.ones_like(hf))
            assert torch.equal(hf @ hf.T, n * torch.eye(n, dtype=torch.float64)), (fn.__name__, n)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "exllamav3")), reason="needs the reference tree")
def test_had_paley_equals_the_reference_torch_builders():
    import importlib.util
    import types
    from exllamav3_amd import ext
    src = open(os.path.join(REF, "exllamav3", "util", "hadamard.py")).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("is_quadratic_residue", "paley_torch", "paley2_torch")]
    mod = types.ModuleType("ref_hadamard_builders")
    mod.torch = torch
    exec(compile(ast.Module(body=keep, type_ignores=[]), "hadamard.py", "exec"), mod.__dict__)
    p1, _, p2_any = _paley_sizes(260)
    for n in p1:
        h = torch.empty((n, n), dtype=torch.half); ext.had_paley(h)
        assert torch.equal(h, mod.paley_torch(n)), n
    for n in p2_any:
        h = torch.empty((n, n), dtype=torch.half); ext.had_paley2(h)
        assert torch.equal(h, mod.paley2_torch(n)), n


def _ext_names(path):
    tree = ast.parse(open(path).read())
    return {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "ext"}


def test_every_quantizer_ext_name_resolves():
    """Against the reference tree where it is present (and then the record must agree with it), else against the record."""
    from exllamav3_amd import ext
    recorded = json.load(open(NAMES_RECORD))
    if os.path.isdir(os.path.join(REF, "exllamav3")):
        now = {m: sorted(_ext_names(os.path.join(REF, "exllamav3", m))) for m in QUANTIZER_MODULES}
        assert now == recorded, "tests/golden/ref_quantizer_ext_names.json is stale"
    assert sorted(recorded) == sorted(QUANTIZER_MODULES)
    missing = {m: sorted(n for n in names if not hasattr(ext, n)) for m, names in recorded.items()}
    assert not any(missing.values()), missing


def test_quantize_tiles_argument_errors_without_gpu():
    from exllamav3_amd import ext, _lib
    n, K = 2, 4
    E = 65536 >> K
    x = torch.zeros((n, 256))
    out = torch.zeros((n, 256))
    idx = torch.zeros((n, 256), dtype=torch.short)
    tc = torch.zeros((1, 2, E), dtype=torch.half)
    te = torch.zeros((1, 256, E), dtype=torch.short)
    with pytest.raises(RuntimeError, match="K must be in range"):
        ext.quantize_tiles(x, out, idx, tc, te, 9, False, False)
    with pytest.raises(RuntimeError, match="K must be in range"):
        ext.quantize_tiles(x, out, idx, tc, te, 0, False, False)
    with pytest.raises(RuntimeError):
        ext.quantize_tiles(x.half(), out, idx, tc, te, K, False, False)
    with pytest.raises(RuntimeError):
        ext.quantize_tiles(x, out, idx.int(), tc, te, K, False, False)
    with pytest.raises(RuntimeError):
        ext.quantize_tiles(x[:, :128], out, idx, tc, te, K, False, False)
    with pytest.raises(RuntimeError):
        ext.quantize_tiles(x, out, idx[:1], tc, te, K, False, False)
    with pytest.raises(RuntimeError):
        ext.quantize_tiles(x, out, idx, tc[:, :, :E // 2], te, K, False, False)
    with pytest.raises(RuntimeError):
        ext.quantize_tiles(x, out, idx, tc, te.int(), K, False, False)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.quantize_tiles(x, out, idx, tc, te, K, False, False)
    # n = 0 is a no-op even on CPU tensors (the reference returns before touching the temp buffers)
    ext.quantize_tiles(x[:0], out[:0], idx[:0], tc, te, K, False, False)
    # the C-ABI rejects K and the codebook before any device work
    assert _lib.lib().exl3_quantize_tiles(None, None, None, 1, None, 1, 9, 0, None) == -1
    assert b"K must be in range 1..8" in _lib.lib().exl3_last_error()
    assert _lib.lib().exl3_quantize_tiles(None, None, None, 1, None, 1, 4, 3, None) == -1
    assert b"bad codebook" in _lib.lib().exl3_last_error()
    # the per-tile workspace: 256 positions x one packed back-pointer word per thread, within one (256, E) int16 slot
    for k in range(1, 9):
        b = ext.quantize_tiles_workspace_bytes(k)
        assert 0 < b <= 256 * (65536 >> k) * 2
        assert b * 8 >= 256 * (65536 >> k) * k
