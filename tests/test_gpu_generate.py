"""Device-side generation (SyntheticEXL3Llama.generate: decode step + sampler + token feed captured once, replayed per token) on 2-layer models of Llama-3.2-1B and
Llama-3.1-8B width, full vocabulary, attention on, empty cache -- against a host-stepped loop built only from alloc_state / decode_step_auto / torch indexing."""
import math
import numpy as np
import pytest
import torch
import _sampler_ref as R

pytestmark = pytest.mark.gpu

V = 128256
WIDTHS = {"1b": (2048, 8192, 32, 8, 64), "8b": (4096, 14336, 32, 8, 128)}
PROMPT = [128000, 9906, 11, 856, 836, 374, 1234, 77]


@pytest.fixture(autouse=True)
def _leave_the_default_generator_as_found(dev):
    """alloc_state draws its input rows from the default device generator; tests that run after this file keep seeing the rows they always saw."""
    state = torch.cuda.get_rng_state(dev)
    yield
    torch.cuda.set_rng_state(state, dev)


@pytest.fixture(scope="module", params=["1b", "8b"])
def model(request, dev):
    from exllamav3_amd import ext
    from exllamav3_amd.llama_path import LlamaShape, SyntheticEXL3Llama
    ext.set_gemv_variant(1)
    hidden, inter, hq, hkv, hd = WIDTHS[request.param]
    m = SyntheticEXL3Llama(LlamaShape("gen-" + request.param, hidden, inter, 2, hq, hkv, hd, V), K=4, cb=2, device=dev, kv_bits=4, max_ctx=512, seed=3)
    yield m
    del m
    torch.cuda.empty_cache()


def _host_loop(m, tokens_in, pick=None):
    """The generation loop stepped from the host with the parent's pieces only: x0 = table[token] (torch indexing), decode_step_auto(), logits copied to the host, the
    counters advanced from the host.  tokens_in: the forced inputs; behind them the loop feeds pick(step, logits).  Returns (tokens fed from step 1 on, logits per step)."""
    table = m.embed_table()
    m.with_attention = True
    m.alloc_state(1, pos=m.max_ctx - 1)
    out, logs = [], []
    tok = tokens_in[0]
    n = len(tokens_in) if pick is None else pick[0]
    for s in range(n):
        m.positions.fill_(s); m.cache_seqlens.fill_(s); m.attn_lens.fill_(s + 1)
        m.x0.copy_(table[tok].view(1, -1))
        l = m.decode_step_auto()[0].cpu().numpy().copy()
        logs.append(l)
        tok = tokens_in[s + 1] if s + 1 < len(tokens_in) else (pick[1](s, l) if pick is not None else -1)
        out.append(tok)
    m.with_attention = False
    return out, logs


def test_feed_forced_tokens_counters_and_invalid_tokens(dev, model):
    from exllamav3_amd import sampling
    m = model
    table = m.embed_table()
    prompt = torch.tensor([PROMPT[:4], [5, 6, 7, V - 1]])
    gs = m.alloc_gen_state(2, 4, prompt)
    # primed: the first prompt token is the input row, counters at the first position, step word 0
    assert torch.equal(m.x0.view(torch.int16), table[prompt[:, 0].to(dev)].view(torch.int16))
    assert m.positions.tolist() == [0, 0] and m.cache_seqlens.tolist() == [0, 0] and m.attn_lens.tolist() == [1, 1] and int(gs.step) == 0
    for s in range(3):                                                   # forced tokens win over the sampled ones while they last
        gs.sampled.fill_(99)
        sampling.gen_feed(gs.sampled, gs.forced, gs.embed, m.x0, gs.tokens_out, m.positions, m.cache_seqlens, m.attn_lens, gs.invalid, gs.step, vocab=V)
        assert gs.tokens_out[:, s].tolist() == prompt[:, s + 1].tolist()
        assert torch.equal(m.x0.view(torch.int16), table[prompt[:, s + 1].to(dev)].view(torch.int16))
        assert m.positions.tolist() == [s + 1] * 2 and m.cache_seqlens.tolist() == [s + 1] * 2 and m.attn_lens.tolist() == [s + 2] * 2 and int(gs.step) == s + 1
    gs.sampled.copy_(torch.tensor([1234, V - 2], dtype=torch.int32))     # the forced list is used up: sampled tokens
    sampling.gen_feed(gs.sampled, gs.forced, gs.embed, m.x0, gs.tokens_out, m.positions, m.cache_seqlens, m.attn_lens, gs.invalid, gs.step, vocab=V)
    assert gs.tokens_out[:, 3].tolist() == [1234, V - 2] and gs.invalid.tolist() == [0, 0]
    assert torch.equal(m.x0.view(torch.int16), table[torch.tensor([1234, V - 2], device=dev)].view(torch.int16))
    before = m.x0.clone()
    gs.sampled.copy_(torch.tensor([-1, 17], dtype=torch.int32))          # -1 (an invalid row of the sampler) never indexes the table
    sampling.gen_feed(gs.sampled, gs.forced, gs.embed, m.x0, gs.tokens_out, m.positions, m.cache_seqlens, m.attn_lens, gs.invalid, gs.step, vocab=V)
    assert gs.tokens_out[:, 4].tolist() == [-1, 17] and gs.invalid.tolist() == [1, 0]
    assert torch.equal(m.x0[0], before[0]) and torch.equal(m.x0[1].view(torch.int16), table[17].view(torch.int16))
    gs.sampled.copy_(torch.tensor([5, V], dtype=torch.int32))            # sticky: row 0 stays invalid whatever comes; `vocab` is out of range too
    sampling.gen_feed(gs.sampled, gs.forced, gs.embed, m.x0, gs.tokens_out, m.positions, m.cache_seqlens, m.attn_lens, gs.invalid, gs.step, vocab=V)
    assert gs.tokens_out[:, 5].tolist() == [-1, -1] and gs.invalid.tolist() == [1, 1]
    assert torch.equal(m.x0[0], before[0]) and torch.equal(m.x0[1].view(torch.int16), table[17].view(torch.int16))
    assert int(gs.step) == 6 and m.positions.tolist() == [6, 6]


def test_greedy_generate_equals_the_host_stepped_loop(dev, model):
    m = model
    got = m.generate(PROMPT, 32)
    assert got.dtype == torch.long and got.shape == (32,)
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": len(PROMPT) - 1 + 32, "host_reads": 1}
    ps = getattr(m, "_pstep", None)
    assert ps is None or not ps.error()
    again = m.generate(PROMPT, 32)
    assert torch.equal(got, again)
    exp, _ = _host_loop(m, PROMPT, pick=(len(PROMPT) - 1 + 32, lambda s, l: int(np.argmax(l[:V].astype(np.float32)))))
    assert got.tolist() == exp[len(PROMPT) - 1:], (got.tolist(), exp[len(PROMPT) - 1:])
    # EOS: trimmed behind the first occurrence on the host
    eos = int(got[5])
    first = got.tolist().index(eos)
    assert m.generate(PROMPT, 32, eos_token_id=eos).tolist() == got.tolist()[:first + 1]


def test_sampled_generate_passes_the_sampler_criterion_step_by_step(dev, model):
    from exllamav3_amd.sampling import SamplerSettings
    m = model
    st = SamplerSettings(temperature=0.8, top_k=50, top_p=0.9, seed=2026)
    ka = st.kernel_args()
    got = m.generate(PROMPT, 32, settings=st)
    assert torch.equal(got, m.generate(PROMPT, 32, settings=st))                                     # same seed: same tokens
    other = m.generate(PROMPT, 32, settings=SamplerSettings(temperature=0.8, top_k=50, top_p=0.9, seed=2027))
    assert not torch.equal(got, other)
    P = len(PROMPT)
    fed, logs = _host_loop(m, PROMPT + got.tolist()[:-1])
    worst = 0.0
    for i, t in enumerate(got.tolist()):
        s = P - 1 + i                                                                                # the step whose logits produced token i
        l = logs[s][:V]
        cut = R.cutoff(l, ka.mode, filters=ka.filters, top_k=ka.top_k, top_p=ka.top_p, inv_temp_filter=ka.inv_temp_filter, minp_log=ka.minp_log)
        v = R.objective(l, ka.inv_temp, 0, s, ka.seed, cut)
        tol = 16 * 2.0 ** -24 * np.abs(v[np.isfinite(v)]).max()
        worst = max(worst, float(v.max() - v[t]))
        assert v[t] >= v.max() - tol, (i, t, int(np.argmax(v)), float(v.max() - v[t]), tol)
    print("sampled generate: largest objective deviation", worst)


def test_loop_is_captured_once_and_replayed_without_host_reads(dev, model, monkeypatch):
    m = model
    events = []
    real_replay, real_cpu, real_item, real_tolist = torch.cuda.CUDAGraph.replay, torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist
    real_sync, real_capture = torch.cuda.synchronize, torch.cuda.CUDAGraph.capture_begin
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (events.append("replay"), real_replay(self))[1])
    monkeypatch.setattr(torch.cuda.CUDAGraph, "capture_begin", lambda self, *a, **k: (events.append("capture"), real_capture(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (events.append("read") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (events.append("read") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (events.append("read") if self.is_cuda else None, real_tolist(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (events.append("sync"), real_sync(*a, **k))[1])
    got = m.generate(PROMPT, 16)
    monkeypatch.undo()
    n = len(PROMPT) - 1 + 16
    assert events.count("capture") == 1 and events.count("replay") == n
    first = events.index("replay")
    assert events[first:first + n] == ["replay"] * n, events[first:]                                 # nothing between the replays
    assert events[first + n:] == ["read"], events[first + n:]                                        # one read at the end
    assert got.shape == (16,)


def test_generate_survives_a_checkpoint_round_trip(dev, tmp_path):
    """save_checkpoint writes the embedding table, from_checkpoint reads it back on demand: the same tokens (the smaller width: the files hold the whole table)."""
    from exllamav3_amd.llama_path import LlamaShape, SyntheticEXL3Llama
    hidden, inter, hq, hkv, hd = WIDTHS["1b"]
    m = SyntheticEXL3Llama(LlamaShape("gen-rt", hidden, inter, 2, hq, hkv, hd, V), K=4, cb=2, device=dev, kv_bits=4, max_ctx=512, seed=4)
    got = m.generate(PROMPT, 16)
    m.save_checkpoint(str(tmp_path))
    m2 = SyntheticEXL3Llama.from_checkpoint(str(tmp_path), device=dev, max_ctx=512)
    assert torch.equal(m2.embed_table().view(torch.int16), m.embed_table().view(torch.int16))
    assert torch.equal(m2.generate(PROMPT, 16), got)


def test_attention_inside_the_step_from_position_zero(dev):
    """Positions 0..5 of an empty, growing cache (below the range the persistent step's own tests cover): the persistent step with the attention inside against the
    launch-per-op pipeline on the same tensors and the same cache, fed through the token feed.  Bar: 2e-2 * RMS, the bar of the existing step-vs-step comparisons."""
    from exllamav3_amd import sampling
    from exllamav3_amd.llama_path import LlamaShape, SyntheticEXL3Llama
    for hd, hq, hkv in ((128, 4, 1), (64, 8, 2)):
        m = SyntheticEXL3Llama(LlamaShape("gen-tiny", 512, 1536, 2, hq, hkv, hd, 1024), K=4, cb=2, device=dev, kv_bits=4, max_ctx=512, seed=5)
        m.with_attention = True
        gs = m.alloc_gen_state(1, 0, torch.tensor([[3, 1000, 17, 512, 99, 7]]))
        assert m.persistent_applies()
        for s in range(6):
            assert m.positions.tolist() == [s] and m.attn_lens.tolist() == [s + 1]
            lf = m.decode_step_fx().float().cpu().numpy().copy()
            lp = m.decode_step_auto().float().cpu().numpy().copy()
            assert m._pstep is not None and not m._pstep.error()
            err = np.abs(lp - lf).max() / (np.sqrt((lf ** 2).mean()) + 1e-9)
            assert np.isfinite(lp).all() and err < 2e-2, (hd, s, err)
            sampling.gen_feed(None, gs.forced, gs.embed, m.x0, None, m.positions, m.cache_seqlens, m.attn_lens, gs.invalid, gs.step, vocab=1024)
