"""Speculative decoding in SyntheticEXL3Llama.generate(speculative=...) on tiny 2-layer models (hidden 512, intermediate 2048, vocabulary 1024, 4 bpw mul1, 4-bit
cache, max_ctx 512; head_dim 64 and 128): 48 new tokens behind a 9-token prompt.  The drafts must never change the tokens: every drafter gives what a host-stepped
loop over the same m-row fused step gives that commits one token per round (built here from alloc_gen_state / ingest_prompt / alloc_state / decode_step_fused)."""
import math
import numpy as np
import pytest
import torch
import _spec_ref as R

pytestmark = pytest.mark.gpu

V, NEW, MAX_CTX = 1024, 48, 512
SHAPES = {"hd64": (512, 2048, 8, 2, 64), "hd128": (512, 2048, 4, 1, 128)}
PROMPT = [3, 1000, 17, 512, 99, 7, 640, 2, 311]
P = len(PROMPT)
_RUNS = {}


@pytest.fixture(autouse=True)
def _leave_the_default_generator_as_found(dev):
    """alloc_state draws its input rows from the default device generator; tests that run after this file keep seeing the rows they always saw."""
    state = torch.cuda.get_rng_state(dev)
    yield
    torch.cuda.set_rng_state(state, dev)


@pytest.fixture(scope="module", params=list(SHAPES))
def model(request, dev):
    from exllamav3_amd import ext
    from exllamav3_amd.llama_path import LlamaShape, SyntheticEXL3Llama
    ext.set_gemv_variant(1)
    hidden, inter, hq, hkv, hd = SHAPES[request.param]
    m = SyntheticEXL3Llama(LlamaShape("spec-" + request.param, hidden, inter, 2, hq, hkv, hd, V), K=4, cb=2, device=dev, kv_bits=4, max_ctx=MAX_CTX, seed=7)
    yield m
    _RUNS.clear()
    del m
    torch.cuda.empty_cache()


def _m_row_state_over_the_ingested_prompt(m, rows):
    """The prompt's first P - 1 tokens through the prefill route into a one-sequence cache (alloc_gen_state + ingest_prompt), then alloc_state's buffers for `rows`
    rows over THAT cache with every block-table row naming its pages."""
    m.with_attention = True
    m.alloc_gen_state(1, 1, torch.tensor([PROMPT]))
    m.ingest_prompt(P - 1)
    kc, vc, bt = m.kcache, m.vcache, m.block_table
    m.alloc_state(rows, pos=m.max_ctx - 1)
    m.kcache, m.vcache, m.block_table = kc, vc, bt.repeat(rows, 1).contiguous()


def _host_rounds(m, k, n_new, ka=None, script=None):
    """The speculative loop stepped from the host over the m-row fused step.  Without a script every row carries the last committed token and row 0's token is
    committed: one token per round.  With a script rows 1 .. c carry its drafts and the accept rule runs here.  ka None: numpy argmax of each row; else
    sampling.sample with the step word = round.  Returns (tokens, rounds)."""
    from exllamav3_amd import sampling
    rows, dev = k + 1, m.device
    _m_row_state_over_the_ingested_prompt(m, rows)
    table = m.embed_table()
    ar = torch.arange(rows, dtype=torch.int32, device=dev)
    stepw = torch.zeros((1,), dtype=torch.int64, device=dev)
    hist, out, rnd = list(PROMPT), [], 0
    while len(out) < n_new:
        base = len(hist) - 1
        d = R.script_draft(script, base + 1, k, V) if script is not None else []
        toks = [hist[-1]] + d + [hist[-1]] * (rows - 1 - len(d))
        m.positions.copy_(base + ar); m.cache_seqlens.copy_(base + ar); m.attn_lens.copy_(base + 1 + ar)
        m.x0.copy_(table[torch.tensor(toks, device=dev)])
        logits = m.decode_step_fused()
        if ka is None:
            s = [int(np.argmax(l[:V].astype(np.float32))) for l in logits.cpu().numpy()]
        else:
            stepw.fill_(rnd)
            s = sampling.sample(logits, ka, stepw, size=V).tolist()
        n = 0
        while n < len(d) and toks[n + 1] == s[n]:
            n += 1
        n = min(n, n_new - len(out) - 1)
        hist += s[:n + 1]; out += s[:n + 1]
        rnd += 1
    m.with_attention = False
    return out, rnd


def _script(tokens, wrong):
    """A draft table by absolute position behind the prompt: tokens[j] at P + j, (tokens[j] + 1) % V where wrong(j)."""
    s = [-1] * P + [(t + 1) % V if wrong(j) else t for j, t in enumerate(tokens)]
    return s + [-1] * (MAX_CTX - len(s))


def _runs(m, k):
    """Per (model, k), computed once: the host loop's tokens and generate() under the four drafters, with their gen_stats."""
    from exllamav3_amd.sampling import SpeculativeSettings
    key = (m.shape.name, k)
    if key not in _RUNS:
        host, rounds = _host_rounds(m, k, NEW)
        assert rounds == NEW
        r = {"host": host}
        drafters = {"oracle": _script(host, lambda j: False), "all_wrong": _script(host, lambda j: True), "two_right_then_wrong": _script(host, lambda j: j % 3 == 2),
                    "ngram": None}
        for name, sc in drafters.items():
            got = m.generate(PROMPT, NEW, speculative=SpeculativeSettings(num_draft_tokens=k, script=sc))
            r[name] = (got.tolist(), dict(m.gen_stats))
        _RUNS[key] = r
    return _RUNS[key]


@pytest.mark.parametrize("rows", [2, 4, 5, 8])
def test_1_fused_step_gives_bit_equal_rows_for_equal_inputs(dev, model, rows):
    """The premise of everything below, a property of the step as it stands: the same token at the same position with the same past in all rows (separate,
    non-aliased caches holding the same content) gives bit-equal logits rows -- on both sides of the change of GEMV kernel generation between 4 and 5 rows."""
    m = model
    m.with_attention = True
    m.alloc_state(rows, pos=40)
    m.x0.copy_(m.x0[0:1].expand(rows, -1).clone())
    for c, s in m.kcache + m.vcache:
        one = torch.randint(-2 ** 31, 2 ** 31 - 1, (c.shape[0] // rows,) + tuple(c.shape[1:]), device=dev, dtype=torch.int64).to(torch.int32)
        c.view(rows, -1).copy_(one.view(1, -1).expand(rows, -1))
        sc = (torch.rand((s.shape[0] // rows,) + tuple(s.shape[1:]), device=dev) * 0.05 + 0.01).half()
        s.view(rows, -1).copy_(sc.view(1, -1).expand(rows, -1))
    logits = m.decode_step_fused().cpu()
    m.with_attention = False
    assert torch.isfinite(logits.float()).all()
    diff = float((logits.float() - logits[0:1].float()).abs().max())
    print(f"row symmetry, {rows} rows: largest |logits[i] - logits[0]| = {diff}")
    assert torch.equal(logits.view(torch.int16), logits[0:1].expand(rows, -1).contiguous().view(torch.int16))


@pytest.mark.parametrize("k", [1, 3, 4, 7])
def test_2_greedy_output_does_not_depend_on_the_drafts(dev, model, k):
    r = _runs(model, k)
    for name in ("oracle", "all_wrong", "two_right_then_wrong", "ngram"):
        toks, _ = r[name]
        assert len(toks) == NEW and toks == r["host"], (name, k, toks, r["host"])


@pytest.mark.parametrize("k", [1, 3, 4, 7])
def test_3_round_counts(dev, model, k):
    r = _runs(model, k)
    for name in ("oracle", "all_wrong", "two_right_then_wrong", "ngram"):
        toks, st = r[name]
        assert st["graph_captures"] == 1 and st["graph_replays"] <= NEW, (name, st)
        assert st["spec_accepted"] + st["spec_rounds"] == len(toks) == NEW, (name, st)
        assert st["spec_accepted"] <= st["spec_drafted"] <= k * st["spec_rounds"], (name, st)
        assert st["prefill_tokens"] == P - 1 and st["host_reads"] >= 1
    st = r["oracle"][1]
    assert st["spec_rounds"] == math.ceil(NEW / (k + 1)) and st["spec_accepted"] == NEW - st["spec_rounds"], st
    st = r["all_wrong"][1]
    assert st["spec_rounds"] == NEW and st["spec_accepted"] == 0 and st["graph_replays"] == NEW, st
    st = r["two_right_then_wrong"][1]
    assert 0 < st["spec_accepted"] < r["oracle"][1]["spec_accepted"] or k == 1, st
    print(f"k = {k}: rounds for {NEW} tokens:", {n: r[n][1]["spec_rounds"] for n in ("oracle", "two_right_then_wrong", "ngram", "all_wrong")})


def test_4_against_plain_generate_on_the_default_step(dev, model):
    """The default step of plain generate() is the persistent step, another kernel family: bit equality is not promised.  Tokens agree up to the first difference,
    if any; there the two tokens are the plain step's top two, and their margin is at most twice the largest absolute difference between the plain step's logits
    and row 0 of the m-row fused step ON THE SAME STATE (the plain step's own cache up to that position) -- a bound measured here, at that step.  Both sides ingest
    the prompt through the prefill route (prompt_mode "prefill"), so they start from the same cache.  The measurement runs at the last token when nothing differs."""
    m, k = model, 3
    spec = _runs(m, k)["oracle"][0]
    plain = m.generate(PROMPT, NEW, prompt_mode="prefill").tolist()
    differ = [j for j in range(NEW) if spec[j] != plain[j]]
    d = differ[0] if differ else NEW - 1
    # the plain step's state in front of new token d: the prompt ingested, then the agreed tokens through decode_step_auto
    m.with_attention = True
    m.alloc_gen_state(1, 1, torch.tensor([PROMPT]))
    m.ingest_prompt(P - 1)
    table = m.embed_table()
    fed = [PROMPT[-1]] + plain[:d]
    for j, tok in enumerate(fed):
        m.positions.fill_(P - 1 + j); m.cache_seqlens.fill_(P - 1 + j); m.attn_lens.fill_(P + j)
        m.x0.copy_(table[tok].view(1, -1))
        lp = m.decode_step_auto()[0].float().cpu().numpy().copy()
    kc, vc, bt = m.kcache, m.vcache, m.block_table
    rows, base = k + 1, P - 1 + d
    m.alloc_state(rows, pos=m.max_ctx - 1)
    m.kcache, m.vcache, m.block_table = kc, vc, bt.repeat(rows, 1).contiguous()
    ar = torch.arange(rows, dtype=torch.int32, device=dev)
    m.positions.copy_(base + ar); m.cache_seqlens.copy_(base + ar); m.attn_lens.copy_(base + 1 + ar)
    m.x0.copy_(table[fed[-1]].view(1, -1).expand(rows, -1))
    lf = m.decode_step_fused()[0].float().cpu().numpy().copy()
    m.with_attention = False
    diff = float(np.abs(lp[:V] - lf[:V]).max())
    order = np.argsort(-lp[:V], kind="stable")
    margin = float(lp[order[0]] - lp[order[1]])
    print(f"first difference: {differ[0] if differ else None}; at new token {d}: |plain - fused row 0| max = {diff}, plain top-two margin = {margin}")
    assert int(order[0]) == plain[d], "the host-stepped plain step does not reproduce plain generate()"
    if differ:
        assert {plain[d], spec[d]} == {int(order[0]), int(order[1])}, (d, plain[d], spec[d], order[:4].tolist())
        assert margin <= 2 * diff, (d, margin, diff)


def test_5_stop_token_cuts_an_oracle_run_behind_it(dev, model):
    from exllamav3_amd.sampling import SpeculativeSettings
    m = model
    truth = _runs(m, 3)["host"]
    k = 3 if (truth.index(truth[5]) + 1) % 4 else 4                      # so that the cut falls inside a round, not on its last row
    truth = _runs(m, k)["host"]
    stop = truth[5]                                                      # the 6th greedy token (or an earlier position, should the token occur there already)
    first = truth.index(stop)
    got = m.generate(PROMPT, NEW, speculative=SpeculativeSettings(num_draft_tokens=k, script=_script(truth, lambda j: False)), stop_token_ids=[stop])
    st = dict(m.gen_stats)
    assert got.tolist() == truth[:first + 1], (got.tolist(), truth[:first + 1])
    assert st["stopped_after"] is not None and st["graph_replays"] < NEW and st["spec_rounds"] == math.ceil((first + 1) / (k + 1)), st
    assert st["spec_accepted"] + st["spec_rounds"] == first + 1
    plain = m.generate(PROMPT, NEW, stop_token_ids=[stop], prompt_mode="prefill")
    assert got.tolist() == plain.tolist(), (got.tolist(), plain.tolist())
    # an EOS id trims the same way
    eos = m.generate(PROMPT, NEW, speculative=SpeculativeSettings(num_draft_tokens=k), eos_token_id=stop)
    assert eos.tolist() == truth[:first + 1]


def test_6_sampled_mode_equals_the_host_stepped_loop(dev, model):
    from exllamav3_amd.sampling import SamplerSettings, SpeculativeSettings
    m, k = model, 3
    st = SamplerSettings(temperature=0.8, top_k=50, top_p=0.9, seed=2026)
    wrong = _script(_runs(m, k)["host"], lambda j: True)                 # wrong for the greedy continuation; a sampled token may still meet a draft
    got = m.generate(PROMPT, NEW, settings=st, speculative=SpeculativeSettings(num_draft_tokens=k, script=wrong))
    stats = dict(m.gen_stats)
    again = m.generate(PROMPT, NEW, settings=st, speculative=SpeculativeSettings(num_draft_tokens=k, script=wrong))
    assert torch.equal(got, again)
    exp, rounds = _host_rounds(m, k, NEW, ka=st.kernel_args(), script=wrong)
    assert got.tolist() == exp, (got.tolist(), exp)
    assert stats["spec_rounds"] == rounds and stats["spec_accepted"] == NEW - rounds
    assert got.tolist() != _runs(m, k)["host"]                           # (it did sample)
    other = m.generate(PROMPT, NEW, settings=SamplerSettings(temperature=0.8, top_k=50, top_p=0.9, seed=2027),
                       speculative=SpeculativeSettings(num_draft_tokens=k, script=wrong))
    assert not torch.equal(got, other)


def test_7_refusals_and_the_default_path(dev, model):
    from exllamav3_amd.sampling import LogitProcessors, SpeculativeSettings
    m = model
    S = SpeculativeSettings(num_draft_tokens=3)
    with pytest.raises(NotImplementedError):
        m.generate(PROMPT, 8, speculative=S, processors=LogitProcessors(rep_p=1.3))
    with pytest.raises(NotImplementedError):
        m.generate([PROMPT, PROMPT], 8, speculative=S)
    with pytest.raises(ValueError):
        m.generate(PROMPT, MAX_CTX - P - 3 + 1, speculative=S)
    with pytest.raises(ValueError):
        m.alloc_spec_state(3, MAX_CTX - P - 3 + 1, PROMPT)
    with pytest.raises(TypeError):
        m.generate(PROMPT, 8, speculative=3)
    got = m.generate(PROMPT, 4)
    assert got.shape == (4,) and set(m.gen_stats) == {"graph_captures", "graph_replays", "host_reads"}
    assert m.generate(PROMPT, 0, speculative=S).numel() == 0
    one = m.generate(PROMPT[:1], 6, speculative=S)                       # a one-token prompt: nothing to ingest
    assert one.shape == (6,) and "prefill_tokens" not in m.gen_stats
