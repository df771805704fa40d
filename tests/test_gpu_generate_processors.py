"""generate() with logit processors and stop tokens, on the 2-layer models of Llama-3.2-1B and Llama-3.1-8B width of test_gpu_generate.py: the replayed device loop
against a host-stepped loop built from alloc_state / decode_step_auto / torch indexing that applies the numpy restatement (tests/_logit_proc_ref.py) to the copied
logits before argmax."""
import numpy as np
import pytest
import torch
import _logit_proc_ref as LP

pytestmark = pytest.mark.gpu

V = 128256
WIDTHS = {"1b": (2048, 8192, 32, 8, 64), "8b": (4096, 14336, 32, 8, 128)}
PROMPT = [128000, 9906, 11, 856, 836, 374, 1234, 77]
PROMPT2 = [128000, 791, 4320, 311, 279, 3488, 374, 25]
NEW = 32


@pytest.fixture(autouse=True)
def _leave_the_default_generator_as_found(dev):
    state = torch.cuda.get_rng_state(dev)
    yield
    torch.cuda.set_rng_state(state, dev)


@pytest.fixture(scope="module", params=["1b", "8b"])
def model(request, dev):
    from exllamav3_amd import ext
    from exllamav3_amd.llama_path import LlamaShape, SyntheticEXL3Llama
    ext.set_gemv_variant(1)
    hidden, inter, hq, hkv, hd = WIDTHS[request.param]
    m = SyntheticEXL3Llama(LlamaShape("genp-" + request.param, hidden, inter, 2, hq, hkv, hd, V), K=4, cb=2, device=dev, kv_bits=4, max_ctx=512, seed=3)
    yield m
    del m
    torch.cuda.empty_cache()


def _host_loop(m, prompt, n_new, pick):
    """The loop stepped from the host with the parent's pieces: x0 = table[token], decode_step_auto(), logits copied to the host, counters advanced from the host.
    Behind the prompt it feeds pick(tokens fed so far, logits row).  Returns the new tokens."""
    table = m.embed_table()
    m.with_attention = True
    m.alloc_state(1, pos=m.max_ctx - 1)
    fed = [prompt[0]]
    for s in range(len(prompt) - 1 + n_new):
        m.positions.fill_(s); m.cache_seqlens.fill_(s); m.attn_lens.fill_(s + 1)
        m.x0.copy_(table[fed[-1]].view(1, -1))
        l = m.decode_step_auto()[0].cpu().numpy().copy()
        fed.append(prompt[s + 1] if s + 1 < len(prompt) else pick(fed, l))
    m.with_attention = False
    return fed[len(prompt):]


def _greedy_after(rep=None, pf=None, bias=None, bitmask=None):
    def pick(fed, l):
        row = LP.process_row(l, V, fed, rep, pf, bias, bitmask, np.float16)
        return int(np.argmax(row[:V].astype(np.float32)))
    return pick


def test_penalties_in_the_loop_equal_the_host_stepped_loop(dev, model):
    from exllamav3_amd.sampling import LogitProcessors
    m = model
    procs = LogitProcessors(rep_p=1.3, rep_sustain=16, rep_decay=8, freq_p=0.3)
    got = m.generate(PROMPT, NEW, processors=procs)
    assert got.shape == (NEW,)
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": len(PROMPT) - 1 + NEW, "host_reads": 1}       # still no read inside the loop
    assert torch.equal(got, m.generate(PROMPT, NEW, processors=procs))
    exp = _host_loop(m, PROMPT, NEW, _greedy_after(rep=(1.3, 16, 8), pf=(0.0, 0.3, 10 ** 8, 0)))
    assert got.tolist() == exp, (got.tolist(), exp)


def test_penalties_that_bite_in_the_loop(dev, model):
    """A synthetic model never repeats a token on its own, so the penalties above have nothing to act on behind the prompt.  Here a bias of 100 lifts one token
    above everything: without penalties the loop repeats it for ever; with a frequency penalty of 50 per occurrence it is level with the rest after two
    occurrences -- the continuation must change there, and must still equal the host-stepped loop."""
    from exllamav3_amd.sampling import LogitProcessors
    m = model
    bias_d = {1111: 100.0}
    only_bias = m.generate(PROMPT, NEW, processors=LogitProcessors(logit_bias=bias_d))
    assert only_bias.tolist() == [1111] * NEW
    procs = LogitProcessors(rep_p=1.3, rep_sustain=16, rep_decay=8, freq_p=50.0, logit_bias=bias_d)
    got = m.generate(PROMPT, NEW, processors=procs)
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": len(PROMPT) - 1 + NEW, "host_reads": 1}
    bias = np.zeros((V,), dtype=np.float32)
    bias[1111] = 100.0
    exp = _host_loop(m, PROMPT, NEW, _greedy_after(rep=(1.3, 16, 8), pf=(0.0, 50.0, 10 ** 8, 0), bias=bias))
    assert got.tolist() == exp, (got.tolist(), exp)
    assert got.tolist()[:2] == [1111, 1111] and got.tolist() != only_bias.tolist(), got.tolist()      # (the penalties did change the continuation)


def test_bias_and_bans_in_the_loop(dev, model):
    from exllamav3_amd.sampling import LogitProcessors
    m = model
    plain = m.generate(PROMPT, NEW).tolist()
    bans = sorted(set(plain[:6]))                                                     # what the unconstrained run wanted first
    bias_d = {int(plain[8]): -4.0, 12345: 6.0, 777: 2.5, V + 9: 3.0}
    procs = LogitProcessors(logit_bias=bias_d, ban_token_ids=bans)
    got = m.generate(PROMPT, NEW, processors=procs)
    assert not set(got.tolist()) & set(bans), (got.tolist(), bans)
    bias = np.zeros((V,), dtype=np.float32)
    for t, v in procs.bias.items():
        if 0 <= t < V:
            bias[t] = v
    exp = _host_loop(m, PROMPT, NEW, _greedy_after(bias=bias))
    assert got.tolist() == exp, (got.tolist(), exp)


def test_bitmask_in_the_loop(dev, model):
    from exllamav3_amd.sampling import LogitProcessors
    m = model
    rng = np.random.default_rng(21)
    keep = rng.choice(V, 1000, replace=False)
    bm = np.zeros((1, (V + 31) // 32), dtype=np.uint32)
    np.bitwise_or.at(bm[0], keep >> 5, (np.uint32(1) << (keep & 31).astype(np.uint32)))
    procs = LogitProcessors(bitmask=torch.from_numpy(bm.view(np.int32)))
    got = m.generate(PROMPT, NEW, processors=procs)
    assert set(got.tolist()) <= set(int(t) for t in keep)
    exp = _host_loop(m, PROMPT, NEW, _greedy_after(bitmask=bm[0]))
    assert got.tolist() == exp, (got.tolist(), exp)


def test_stop_tokens_end_the_loop_early(dev, model):
    m = model
    P = len(PROMPT)
    plain = m.generate(PROMPT, NEW)
    stop = int(plain[5])
    first = plain.tolist().index(stop)
    by_eos = m.generate(PROMPT, NEW, eos_token_id=stop)
    got = m.generate(PROMPT, NEW, stop_token_ids=[stop], stop_check_every=4)
    assert got.tolist() == by_eos.tolist() == plain.tolist()[:first + 1]
    stop_replay = P + first                                                           # replays behind which the stop token has been taken
    replays = -(-stop_replay // 4) * 4
    assert replays < P - 1 + NEW
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": replays, "host_reads": replays // 4 + 1, "stopped_after": replays}
    # a stop id inside the prompt does not stop; the default check interval is 16
    got = m.generate(PROMPT, NEW, stop_token_ids=[PROMPT[3], stop])
    first2 = min(i for i, t in enumerate(plain.tolist()) if t in (PROMPT[3], stop))
    assert got.tolist() == plain.tolist()[:first2 + 1] and m.gen_stats["graph_replays"] == 16 and m.gen_stats["host_reads"] == 2
    # a stop id that never comes: the whole budget, every check read
    never = next(t for t in range(1000, 2000) if t not in plain.tolist())
    got = m.generate(PROMPT, NEW, stop_token_ids=[never], stop_check_every=8)
    assert got.tolist() == plain.tolist()
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": P - 1 + NEW, "host_reads": (P - 1 + NEW - 1) // 8 + 1, "stopped_after": None}
    with pytest.raises(ValueError):
        m.generate(PROMPT, NEW, stop_token_ids=list(range(65)))
    with pytest.raises(ValueError):
        m.generate(PROMPT, NEW, stop_check_every=4)


def test_stop_tokens_in_a_batch(dev, model):
    m = model
    P = len(PROMPT)
    prompts = [PROMPT, PROMPT2]
    plain = m.generate(prompts, NEW)
    assert plain.shape == (2, NEW)
    stops = [int(plain[0, 4]), int(plain[1, 9])]
    first = [min(i for i, t in enumerate(plain[r].tolist()) if t in stops) for r in range(2)]
    got = m.generate(prompts, NEW, stop_token_ids=stops, stop_check_every=4)
    assert got.shape == (2, NEW)
    for r in range(2):                                                                # each row cut at its own stop, the pad (the first stop id) behind it
        assert got[r].tolist() == plain[r].tolist()[:first[r] + 1] + [stops[0]] * (NEW - first[r] - 1), (r, got[r].tolist(), plain[r].tolist())
    replays = -(-(P + max(first)) // 4) * 4                                           # the loop ends when both rows are done
    assert replays < P - 1 + NEW
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": replays, "host_reads": replays // 4 + 1, "stopped_after": replays}


def test_generate_without_the_new_arguments_is_unchanged(dev, model):
    from exllamav3_amd.sampling import LogitProcessors
    m = model
    got = m.generate(PROMPT, NEW)
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": len(PROMPT) - 1 + NEW, "host_reads": 1}
    exp = _host_loop(m, PROMPT, NEW, lambda fed, l: int(np.argmax(l[:V].astype(np.float32))))
    assert got.tolist() == exp
    # processors that collapse to nothing take the same path: no second buffer, no extra launch
    again = m.generate(PROMPT, NEW, processors=LogitProcessors(rep_p=1.0, logit_bias={5: 0.0}))
    assert torch.equal(got, again) and m.gen.proc_logits is None
    assert m.gen_stats == {"graph_captures": 1, "graph_replays": len(PROMPT) - 1 + NEW, "host_reads": 1}
