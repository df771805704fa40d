"""The persistent decode step with its rectangles cut in whole SIMD rows and the age groups' shares kept per op kind (exl3_pstep.hip: wave_partition / wave_shares), on the
GPU: ONE layer of the Llama-3.1-8B shape (hidden 4096, intermediate 14336) + a 2048-column head -- the bench pin model; smaller models never get a weighted rectangle --
through decode_step_persistent against decode_step_fx on the same tensors, at the default shares and at one non-default pair per kind (gate|up, down, lm_head).  The
2048-column head is cut into one-column rectangles, which always keep the uniform partition (all twelve waves' rows belong to the one column), so the lm_head's pair is
also run over the same layer with a 40960-column head, whose 320 column blocks give a 256-CU chip rectangles of two columns.  Another
cut regroups a rectangle's partial sums among the twelve streaming waves: fp32 summation order only, so the bound is the one tests/test_gpu_pstep.py holds this pair of
pipelines to (2e-2 of the logits' RMS); no time-out, hipGraph replay == eager bits."""
import ctypes
import os
import numpy as np
import pytest
import torch
from test_gpu_fullsize import _np, _relerr, _replay_equals

pytestmark = pytest.mark.gpu

ENV = ("EXL3_HIP_PSTEP_SHARES", "EXL3_HIP_PSTEP_SHARES_DOWN", "EXL3_HIP_PSTEP_SHARES_HEAD")
DEFAULT = {}
# (one kind moved, the other two held at 460,370 whatever their defaults are: plan kind whose cut must differ from the default plan's)
SETTINGS = {"default": ("pin", DEFAULT, None),
            "gate_up": ("pin", {ENV[0]: "400,350", ENV[1]: "460,370", ENV[2]: "460,370"}, 2),
            "down": ("pin", {ENV[1]: "600,300"}, 3),
            "head": ("pin", {ENV[2]: "400,350"}, None),
            "wide_head": ("wide", {ENV[2]: "400,350"}, 4)}
WIDE_VOCAB = 40960


def _reference(m):
    """The input drawn from a generator of its own (not the global device generator: the result must not depend on what ran before), then the launch-per-op
    pipeline's logits, computed once per model."""
    g = torch.Generator(device="cpu").manual_seed(20250607)
    m.x0.copy_(torch.randn(tuple(m.x0.shape), generator=g).half().to(m.x0.device))
    m.x.copy_(m.x0)
    assert m.persistent_applies() and m.shape.hidden == 4096 and m.shape.inter == 14336 and m.n_layers == 1
    for c, s_ in m.kcache + m.vcache: c.zero_(); s_.zero_()
    lf = _np(m.decode_step_fx().float()).copy()
    assert np.isfinite(lf).all()
    return m, lf


@pytest.fixture(scope="module")
def pin(dev):
    from exllamav3_amd import ext
    from exllamav3_amd.llama_path import SyntheticEXL3Llama
    ext.set_gemv_variant(1)
    m = SyntheticEXL3Llama.pin_model("llama-3.1-8b", 4, 2, dev)
    assert m.shape.vocab == 2048
    return _reference(m)


@pytest.fixture(scope="module")
def wide(dev):
    from exllamav3_amd import ext
    from exllamav3_amd.llama_path import LlamaShape, SyntheticEXL3Llama
    ext.set_gemv_variant(1)
    m = SyntheticEXL3Llama(LlamaShape("8b-1layer-wide-head", 4096, 14336, 1, 32, 8, 128, WIDE_VOCAB), K=4, cb=2, device=dev, kv_bits=4, max_ctx=1024)
    m.alloc_state(1, pos=700)
    return _reference(m)


def _cuts(m, kind):
    from exllamav3_amd import _lib
    ncu = torch.cuda.get_device_properties(m.device).multi_processor_count
    s = m.shape
    tiles = np.zeros((ncu, 12), dtype=np.int32); S = ctypes.c_int(0)
    assert _lib.lib().exl3_pstep_plan_tiles(s.hidden, s.inter, s.heads_q, s.heads_kv, s.head_dim, s.vocab, ncu, kind, tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(S)) == 0
    return tiles[tiles[:, 0] >= 0][:, 9:12].copy()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_persistent_step_at_other_cuts_matches_the_launch_per_op_step(request, setting):
    model, env, kind = SETTINGS[setting]
    m, lf = request.getfixturevalue(model)
    saved = {k: os.environ.pop(k, None) for k in ENV}
    try:
        base = {k: _cuts(m, k) for k in (2, 3, 4)}
        for k in (2, 3, 4):                                                  # weighted rectangles of every kind (the lm_head's: the wide head only), cut in whole SIMD rows
            assert base[k].any() == (k != 4 or model == "wide") and not (base[k] & 3).any(), k
        os.environ.update(env)
        if kind is not None:
            assert not np.array_equal(_cuts(m, kind), base[kind]) and _cuts(m, kind).any()
        m._pstep = None                                                      # a new plan: the planner reads the shares when it is made
        for c, s_ in m.kcache + m.vcache: c.zero_(); s_.zero_()
        lp = _np(m.decode_step_persistent().float()).copy()
        assert m._pstep is not None and not m._pstep.error()
        err = _relerr(lp, lf)
        print("setting %s: persistent vs launch-per-op %.5f" % (setting, err))
        assert np.isfinite(lp).all() and err < 2e-2, err
        _replay_equals(m.decode_step_persistent, m, lp, reps=3)
        assert not m._pstep.error()
    finally:
        m._pstep = None
        for k in ENV: os.environ.pop(k, None)
        for k, v in saved.items():
            if v is not None: os.environ[k] = v
