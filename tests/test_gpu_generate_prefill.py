"""generate(prompt_mode="prefill"): the prompt goes through the prefill route in chunks (SyntheticEXL3Llama.ingest_prompt over exl3_embed_rows and the kernels of
prefill_chunk) into the generation's own cache, one feed hands the state over to the replayed loop.  Models of the widths of test_gpu_generate.py (so that plans
and build products are shared) and the small oracle-sized models of test_gpu_attn_prefill.py."""
import os, sys
import numpy as np
import pytest
import torch
import _logit_proc_ref as LP

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import exl3_oracle as o

pytestmark = pytest.mark.gpu

V = 128256
WIDTHS = {"1b": (2048, 8192, 32, 8, 64), "8b": (4096, 14336, 32, 8, 128)}
PROMPT = [128000, 9906, 11, 856, 836, 374, 1234, 77]
NEW = 16


@pytest.fixture(autouse=True)
def _leave_the_default_generator_as_found(dev):
    state = torch.cuda.get_rng_state(dev)
    yield
    torch.cuda.set_rng_state(state, dev)


def _wide(name, width, layers, dev, seed=3):
    from exllamav3_amd import ext
    from exllamav3_amd.llama_path import LlamaShape, SyntheticEXL3Llama
    ext.set_gemv_variant(1)
    hidden, inter, hq, hkv, hd = WIDTHS[width]
    return SyntheticEXL3Llama(LlamaShape(name + width, hidden, inter, layers, hq, hkv, hd, V), K=4, cb=2, device=dev, kv_bits=4, max_ctx=512, seed=seed)


@pytest.fixture(scope="module", params=["1b", "8b"])
def model(request, dev):
    m = _wide("gen-", request.param, 2, dev)
    yield m
    del m
    torch.cuda.empty_cache()


def _long_prompt(n, seed, rows=None):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, V, (n,) if rows is None else (rows, n)))


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- 1. exl3_embed_rows ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bsz", [1, 16])
@pytest.mark.parametrize("hidden,T,col0", [(2048, 1, 0), (72, 13, 7), (4096, 37, 11)])
def test_embed_rows_equals_the_table_rows_bit_for_bit(dev, bsz, hidden, T, col0):
    from exllamav3_amd import sampling
    vocab, ld = 1000, 50
    g = torch.Generator(device=dev); g.manual_seed(bsz * 100 + T)
    table = torch.randn((vocab + 3, hidden), device=dev, generator=g).half()            # rows behind `vocab` must never be read as valid
    ids = torch.randint(0, vocab, (bsz, ld), device=dev, generator=g).to(torch.int32)
    invalid = torch.zeros((bsz,), dtype=torch.int32, device=dev)
    out = sampling.embed_rows(ids, col0, T, table, invalid, vocab=vocab)
    assert out.shape == (bsz * T, hidden) and out.dtype == torch.half
    exp = table[ids[:, col0:col0 + T].long().reshape(-1)]
    assert torch.equal(_bits(out), _bits(exp))
    assert invalid.tolist() == [0] * bsz
    # out-of-range ids: inside the column range a zero row and the row's own invalid flag; outside the range nothing
    bad_row = bsz - 1
    ids2 = ids.clone()
    ids2[bad_row, col0 + T - 1] = vocab                                                 # (== vocab: the first id outside; the table has rows there)
    ids2[0, col0 + T] = -5                                                              # a bad id outside the column range: never looked at
    out2 = torch.full((bsz * T, hidden), float("nan"), dtype=torch.half, device=dev)
    sampling.embed_rows(ids2, col0, T, table, invalid, vocab=vocab, out=out2)
    exp2 = exp.clone()
    exp2[bad_row * T + T - 1] = 0
    assert torch.equal(_bits(out2), _bits(exp2))
    assert invalid.tolist() == [0] * bad_row + [1], invalid.tolist()
    ids3 = ids.clone()
    ids3[0, col0] = -1
    sampling.embed_rows(ids3, col0, T, table, invalid, vocab=vocab, out=out2)         # sticky: the entry sets, never clears
    assert invalid[bad_row].item() == 1 and invalid[0].item() == 1
    assert not out2[0].any()


# ---- 2. same bits as prefill_chunk where the work is the same ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["1b", "8b"])
def test_one_chunk_leaves_the_cache_bits_of_prefill_chunk(dev, width):
    """One layer, bsz 1, one chunk of 300 tokens: the kernels, shapes and inputs of ingest_prompt and prefill_chunk are the same, so the quantised K / V rows
    (words and scales) are compared with no tolerance.  (1b: head_dim 64, three linears + rope; 8b: head_dim 128, the fused q|k|v GEMM + rope_strided.)"""
    T = 300
    m = _wide("gen1-", width, 1, dev)
    prompt = _long_prompt(T + 1, 5)
    gs = m.alloc_gen_state(1, 1, prompt.view(1, -1))
    rows = m.embed_table()[prompt[:T].to(dev)]
    m.prefill_chunk(T)                                                                 # allocates the chunk state (random px0) ...
    m.px0 = rows.clone()                                                               # ... whose input rows become the prompt's
    for t in m.pf_cache:
        t.zero_()
    m.prefill_chunk(T)
    assert m.ingest_prompt(T, chunk=T) == 1
    assert m.cache_seqlens.tolist() == [T] and m.positions.tolist() == [T] and m.attn_lens.tolist() == [T + 1]
    assert int(gs.invalid.sum()) == 0
    (kc, ks), (vc, vs) = m.kcache[0], m.vcache[0]
    pk, pv, pks, pvs = m.pf_cache
    for got, ref, nm in ((kc, pk, "k words"), (vc, pv, "v words")):
        assert torch.equal(got[:2].reshape(512, -1)[:T], ref.reshape(512, -1)[:T]), nm
    for got, ref, nm in ((ks, pks, "k scales"), (vs, pvs, "v scales")):
        assert torch.equal(_bits(got[:2].reshape(512, -1)[:T]), _bits(ref.reshape(512, -1)[:T])), nm
    assert bool(kc[:2].reshape(512, -1)[:T].any()) and not bool(kc[:2].reshape(512, -1)[T:].any())
    del m
    torch.cuda.empty_cache()


# ---- the oracle composition of test_prefill_chunk_with_attention_matches_oracle, per layer, at any head_dim ---------------------------------------------------------
_np = lambda t: t.detach().cpu().numpy()


def _oracle_layer(model, L, x):
    """One transformer layer over all T rows of x (one sequence from position 0): the composition of tests/test_gpu_attn_prefill.py."""
    T, hd = x.shape[0], model.shape.head_dim
    lin = lambda l, a, **kw: o.linear_forward(a, _np(l.trellis), _np(l.suh), _np(l.svh), l.K, 1 if l.mcg else (2 if l.mul1 else 0), **kw)
    xn = o.rms_norm(x, _np(L["norm1"]), model.eps)
    q, k, v = lin(L["q"], xn), lin(L["k"], xn), lin(L["v"], xn)
    q4, k4 = o.rope(q.reshape(1, T, model.hq, hd), k.reshape(1, T, model.hkv, hd), _np(model.inv_freq), position=0, rope_mode=o.ROPE_NEOX)
    kq, ks = o.kv_quant(k4.reshape(T, -1), 4); vq, vs = o.kv_quant(v.reshape(T, -1), 4)
    kd = o.kv_dequant(kq, ks, 4).reshape(1, T, model.hkv, hd); vd = o.kv_dequant(vq, vs, 4).reshape(1, T, model.hkv, hd)
    ao = o.attn_prefill(q4, kd, vd, np.array([T]))
    ov = lin(L["o"], ao.reshape(T, -1), out_fp32=True)
    xn2, x1 = o.rms_norm(ov, _np(L["norm2"]), model.eps, residual_in=x)
    gf, uf = lin(L["gate"], xn2).astype(np.float32), lin(L["up"], xn2).astype(np.float32)
    a = (gf / (1 + np.exp(-gf)) * uf).astype(np.float16)
    d = lin(L["down"], a, out_fp32=True)
    return (x1.astype(np.float32) + d).astype(np.float16)


_rel = lambda g, r: float(np.abs(g.astype(np.float32) - r.astype(np.float32)).max() / np.sqrt((r.astype(np.float32) ** 2).mean()))


# ---- 3. chunked ingestion against the oracle -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bsz", [1, 2])
def test_chunked_ingestion_matches_the_oracle_on_every_row(dev, bsz):
    """The one-layer model of test_prefill_chunk_with_attention_matches_oracle, 299 prompt tokens in chunks of 160: a 160-row chunk on the GEMM route, then a
    139-row chunk on the small-m route that continues a context and crosses the 256-row page boundary.  The oracle runs the whole prompt at once (causal attention
    makes the chunking invisible to it).  Bound: that test's own, 3e-2 of the RMS (same ops, same input statistics).  bsz 2: two different prompts -- rows must
    not leak into each other's pages."""
    from exllamav3_amd.llama_path import LlamaShape, SyntheticEXL3Llama
    vocab, n = 384, 299
    model = SyntheticEXL3Llama(LlamaShape("tiny", 256, 512, 1, 4, 2, 128, vocab), K=4, cb=2, device=dev, kv_bits=4, max_ctx=512)
    rng = np.random.default_rng(17)
    prompt = torch.from_numpy(rng.integers(0, vocab, (bsz, n + 1)))
    gs = model.alloc_gen_state(bsz, 1, prompt)
    got = model.ingest_prompt(n, chunk=160, return_rows=True)
    assert got.shape == (bsz, n, 256) and int(gs.invalid.sum()) == 0
    table = _np(model.embed_table())
    for b in range(bsz):
        ref = _oracle_layer(model, model.layers[0], table[prompt[b, :n].numpy()])
        g = _np(got[b])
        assert np.isfinite(g).all()
        err = _rel(g, ref)
        print(f"chunked ingestion bsz {bsz} row {b}: max-abs error / RMS = {err:.4g} (whole), {_rel(g[160:], ref[160:]):.4g} (second chunk)")
        assert err < 3e-2, (b, err)
    # the cache holds every prompt row of every sequence and nothing behind it
    kc = model.kcache[0][0]
    pps = model.max_ctx // model.page
    for b in range(bsz):
        rows = kc[b * pps:(b + 1) * pps].reshape(pps * model.page, -1)
        assert bool(rows[:n].any(dim=1).all()) and not bool(rows[n:].any())


# ---- 4. the hand-off is exact --------------------------------------------------------------------------------------------------------------------------------------
def test_hand_off_state_equals_decode_mode_integer_for_integer(dev, model):
    from exllamav3_amd import sampling
    m = model
    P, bsz = 40, 2
    prompt = _long_prompt(P, 9, rows=bsz)
    ka = sampling.SamplerSettings(temperature=0.0).kernel_args()
    m.with_attention = True
    try:
        gs = m.alloc_gen_state(bsz, NEW, prompt)
        for _ in range(P - 1):                                                         # decode mode: P - 1 passes of the loop body
            m.gen_step(ka)
        snap = lambda: (int(gs.step), m.positions.tolist(), m.cache_seqlens.tolist(), m.attn_lens.tolist(), gs.tokens_out[:, :P - 1].tolist(),
                        _bits(m.x0).clone(), gs.invalid.tolist())
        dec = snap()
        assert dec[0] == P - 1 and dec[1] == [P - 1] * bsz and dec[3] == [P] * bsz and dec[4] == prompt[:, 1:].tolist()
        chunks = m._gen_prime_prefilled(16)
        pre = snap()
    finally:
        m.with_attention = False
    assert chunks == 3                                                                 # 39 tokens: 16 + 16 + 7
    for a, b, nm in zip(dec[:5], pre[:5], ("step", "positions", "cache_seqlens", "attn_lens", "tokens_out")):
        assert a == b, nm
    assert torch.equal(dec[5], pre[5])                                                 # x0: an embedding row, bit for bit
    assert pre[6] == [0] * bsz
    got = m.generate(prompt, NEW, prompt_mode="prefill", prefill_chunk=16)
    assert got.shape == (bsz, NEW)
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": NEW, "host_reads": 1, "prefill_tokens": bsz * (P - 1), "prefill_chunks": 3}
    assert torch.equal(got, m.generate(prompt, NEW, prompt_mode="prefill", prefill_chunk=16))
    m.generate(prompt, NEW, prompt_mode="prefill")                                     # the default chunk: one chunk
    assert m.gen_stats["prefill_chunks"] == 1 and m.gen_stats["graph_replays"] == NEW


# ---- 5. the first new token's logits, both modes against the oracle --------------------------------------------------------------------------------------------------
#: bound on (prefill mode's error) / (decode mode's error), both against the CPU oracle's logits: the next power of two above the measured ratio, at most 4
F = 2.0


def test_first_new_token_logits_prefill_mode_against_decode_mode(dev):
    """Four layers, hidden 512, head_dim 64, P = 300, greedy: self.logits behind the first replay that samples a new token, in both modes, against the CPU
    oracle's logits for the same model and prompt (max-abs error over the oracle's RMS).  Both must be finite and prefill mode's error within a factor F of
    decode mode's.  Tokens are not compared across modes (synthetic weights give noise-like logits with small top-1 margins; the two GEMM routes round
    differently).
    Measured on an MI355X: decode mode 3.596e-3, prefill mode 3.596e-3 (ratio 1.000; both are one fp16 step of the largest logit over the oracle's RMS), the
    two modes 3.146e-3 apart -> F = 2, the next power of two above the ratio."""
    from exllamav3_amd.llama_path import LlamaShape, SyntheticEXL3Llama
    vocab, P = 1024, 300
    m = SyntheticEXL3Llama(LlamaShape("tiny4", 512, 1536, 4, 8, 2, 64, vocab), K=4, cb=2, device=dev, kv_bits=4, max_ctx=512, seed=11)
    rng = np.random.default_rng(23)
    prompt = torch.from_numpy(rng.integers(0, vocab, (P,)))
    m.generate(prompt, 1)
    assert m.gen_stats["graph_replays"] == P
    l_dec = m.logits[0, :vocab].float().cpu().numpy().copy()
    m.generate(prompt, 1, prompt_mode="prefill", prefill_chunk=160)                     # 299 tokens: 160 (GEMM route) + 139 (small-m route, a continued context)
    assert m.gen_stats["graph_replays"] == 1 and m.gen_stats["prefill_chunks"] == 2
    l_pre = m.logits[0, :vocab].float().cpu().numpy().copy()
    x = _np(m.embed_table())[prompt.numpy()]
    for L in m.layers:
        x = _oracle_layer(m, L, x)
    xl = o.rms_norm(x[-1:], _np(m.final_norm), m.eps)
    h = m.lm_head
    ref = o.linear_forward(xl, _np(h.trellis), _np(h.suh), _np(h.svh), h.K, 1 if h.mcg else (2 if h.mul1 else 0)).astype(np.float32)[0, :vocab]
    assert np.isfinite(l_dec).all() and np.isfinite(l_pre).all()
    e_dec, e_pre = _rel(l_dec, ref), _rel(l_pre, ref)
    print(f"first new token's logits against the oracle: decode mode {e_dec:.4g}, prefill mode {e_pre:.4g}, ratio {e_pre / e_dec:.3f}, "
          f"between the modes {_rel(l_pre, l_dec):.4g}")
    assert np.isfinite(e_dec) and np.isfinite(e_pre)
    assert e_pre <= F * e_dec, (e_pre, e_dec)


# ---- 6. processors and stop tokens ride along ------------------------------------------------------------------------------------------------------------------------
def test_processors_and_stop_tokens_see_the_prefilled_history(dev, model):
    """Greedy with a repetition penalty whose window covers the prompt, a frequency penalty and a bias of 100 on a token the prompt holds twice, plus one stop id:
    the tokens equal those of a loop stepped from the host that starts from the same prefilled state and applies the numpy restatement of the processors to the
    history prompt + fed tokens.  Without the prompt in the history the biased token would win the first step (100 against 100 - 2 * 60 with it): this proves the
    history hand-off, not the numerics of ingestion."""
    from exllamav3_amd.sampling import LogitProcessors
    m = model
    P, hot = 40, 4242
    prompt = _long_prompt(P, 13).tolist()
    prompt[5] = prompt[20] = hot
    rep, pf = (1.3, 64, 8), (0.0, 60.0, 10 ** 8, 0)
    procs = LogitProcessors(rep_p=rep[0], rep_sustain=rep[1], rep_decay=rep[2], freq_p=pf[1], logit_bias={hot: 100.0})
    bias = np.zeros((V,), dtype=np.float32)
    bias[hot] = 100.0
    assert m.generate(prompt, 2, processors=LogitProcessors(logit_bias={hot: 100.0}), prompt_mode="prefill", prefill_chunk=16).tolist() == [hot, hot]
    # the host-stepped loop from the same prefilled state
    table = m.embed_table()
    m.with_attention = True
    try:
        m.alloc_gen_state(1, NEW, torch.tensor([prompt]))
        m._gen_prime_prefilled(16)
        fed, exp = list(prompt), []
        for s in range(P - 1, P - 1 + NEW):
            assert m.positions.tolist() == [s]
            l = m.decode_step_auto()[0].cpu().numpy().copy()
            row = LP.process_row(l, V, fed, rep, pf, bias, None, np.float16)
            tok = int(np.argmax(row[:V].astype(np.float32)))
            fed.append(tok); exp.append(tok)
            m.positions.fill_(s + 1); m.cache_seqlens.fill_(s + 1); m.attn_lens.fill_(s + 2)
            m.x0.copy_(table[tok].view(1, -1))
    finally:
        m.with_attention = False
    assert exp[0] != hot
    got = m.generate(prompt, NEW, processors=procs, prompt_mode="prefill", prefill_chunk=16)
    assert got.tolist() == exp, (got.tolist(), exp)
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": NEW, "host_reads": 1, "prefill_tokens": P - 1, "prefill_chunks": 3}
    stop = exp[5]
    first = exp.index(stop)
    got = m.generate(prompt, NEW, processors=procs, stop_token_ids=[stop], stop_check_every=4, prompt_mode="prefill", prefill_chunk=16)
    assert got.tolist() == exp[:first + 1], (got.tolist(), exp)
    replays = -(-(first + 1) // 4) * 4                                                  # the stop token is taken by replay first + 1; the live word is read every 4
    assert m.gen_stats["graph_replays"] == min(replays, NEW) and m.gen_stats["prefill_tokens"] == P - 1


# ---- 7. interface ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_interface_single_token_prompt_bad_mode_and_tensor_parallel(dev, model):
    m = model
    dec = m.generate(PROMPT[:1], NEW)
    stats = dict(m.gen_stats)
    assert stats == {"graph_captures": 1, "graph_replays": NEW, "host_reads": 1}
    pre = m.generate(PROMPT[:1], NEW, prompt_mode="prefill")                           # nothing to ingest: decode mode
    assert torch.equal(dec, pre) and m.gen_stats == stats
    with pytest.raises(ValueError):
        m.generate(PROMPT, NEW, prompt_mode="chunked")
    with pytest.raises(ValueError):
        m.generate(PROMPT, NEW, prompt_mode="prefill", prefill_chunk=0)
    m.tp = 2
    try:
        with pytest.raises(NotImplementedError):
            m.generate(PROMPT, NEW, prompt_mode="prefill")
        with pytest.raises(NotImplementedError):
            m.ingest_prompt(4)
    finally:
        m.tp = 1
    # a short prompt in prefill mode: same shape of result, the replay count of the new tokens only
    got = m.generate(PROMPT, NEW, prompt_mode="prefill")
    assert got.shape == (NEW,) and m.gen_stats["graph_replays"] == NEW and m.gen_stats["prefill_tokens"] == len(PROMPT) - 1
