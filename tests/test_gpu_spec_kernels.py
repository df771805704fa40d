"""The speculative-decoding kernels (csrc/exl3_spec.hip: exl3_spec_accept, exl3_spec_draft_ngram, exl3_spec_round) against the numpy references of
tests/_spec_ref.py: the n-gram drafter on random histories with planted repeats, the scripted drafter, the feed (input rows bit-equal to the table's), the accept
rule with its cuts, and whole rounds against a toy target."""
import numpy as np
import pytest
import torch
import _spec_ref as R

pytestmark = pytest.mark.gpu

VOCAB, HIDDEN, MAX_CTX = 1024, 64, 4160
I32 = torch.int32


@pytest.fixture(scope="module")
def table(dev):
    g = torch.Generator(device="cpu"); g.manual_seed(11)
    return torch.randn((VOCAB, HIDDEN), generator=g).half().to(dev)


class Dev:
    """The device buffers of one speculative state with m rows."""

    def __init__(self, dev, m, max_new, max_ctx=MAX_CTX):
        self.m, self.max_new = m, max_new
        self.hist = torch.full((max_ctx,), -1, dtype=I32, device=dev)
        self.state = torch.zeros((R.STATE_WORDS,), dtype=I32, device=dev)
        self.round = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.in_tokens = torch.full((m,), -7, dtype=I32, device=dev)
        self.sampled = torch.full((m,), -1, dtype=I32, device=dev)
        self.tokens_out = torch.full((max(max_new, 1),), -1, dtype=I32, device=dev)
        self.x0 = torch.zeros((m, HIDDEN), dtype=torch.half, device=dev)
        self.pos, self.seq, self.lens = (torch.full((m,), -5, dtype=I32, device=dev) for _ in range(3))

    def snapshot(self):
        return {k: getattr(self, k).cpu().clone() for k in ("hist", "state", "round", "in_tokens", "tokens_out", "x0", "pos", "seq", "lens")}


def _set(t, values):
    t.copy_(torch.as_tensor(np.asarray(values), dtype=t.dtype))


def _histories(L, rng):
    """Committed histories of length L (positions behind L hold a copy of the suffix: a kernel reading past L would find matches there)."""
    out = []
    small = rng.integers(0, 3, MAX_CTX)                                            # three symbols: matches of every length, many of them equal
    out.append(small)
    big = rng.integers(0, VOCAB, MAX_CTX)                                          # no repeats to speak of: no draft at match_min >= 2
    out.append(big.copy())
    if L >= 8:
        planted = big.copy()
        n = min(20, L // 3)                                                        # the suffix of n tokens occurred before, twice, the later copy followed by other tokens
        for at in (L // 5, L // 2):
            planted[at:at + n] = planted[L - n:L]
        out.append(planted)
        if L >= 40:
            later_short = big.copy()                                               # a long match early, a short one later: the long one wins
            later_short[2:19] = later_short[L - 17:L]
            later_short[L - 12:L - 9] = later_short[L - 3:L]
            out.append(later_short)
    for h in out:
        h[L:L + 24] = h[max(L - 24, 0):L][:24] if L >= 24 else h[0]
    return out


@pytest.mark.parametrize("L", [1, 2, 3, 17, 255, 256, 257, 4096])
def test_ngram_draft_and_feed_against_the_reference(dev, table, L):
    from exllamav3_amd import sampling
    rng = np.random.default_rng(1000 + L)
    drafted = 0
    for hist in _histories(L, rng):
        for k in (1, 3, 4, 15):
            for m in sorted({k + 1, min(k + 3, 16)}):                              # with and without padding rows behind the k drafts
                for mn, mx in ((1, 1), (2, 8), (16, 16)):
                    d = Dev(dev, m, 64)
                    _set(d.hist, hist)
                    st = np.zeros(R.STATE_WORDS, dtype=np.int64); st[R.BASE], st[R.LIVE], st[R.NDRAFT] = L - 1, 1, 9
                    _set(d.state, st)
                    sampling.spec_draft(d.hist, d.state, d.in_tokens, table, d.x0, d.pos, d.seq, d.lens, k, 64, mn, mx)
                    toks, nd, pos, lens = R.feed(hist, st, m, k, 64, VOCAB, mn, mx)
                    got = d.snapshot()
                    assert got["in_tokens"].tolist() == toks, (L, k, m, mn, mx, got["in_tokens"].tolist(), toks)
                    exp_state = st.copy(); exp_state[R.NDRAFT] = nd
                    assert got["state"].tolist() == exp_state.tolist()
                    assert got["pos"].tolist() == pos and got["seq"].tolist() == pos and got["lens"].tolist() == lens
                    assert torch.equal(got["x0"].view(torch.int16), table[torch.tensor(toks, device=dev)].cpu().view(torch.int16))
                    assert all(t == toks[0] for t in toks[nd + 1:])                # padding rows carry row 0's token
                    assert int(got["round"]) == 0 and torch.equal(got["hist"], torch.as_tensor(hist, dtype=I32))
                    drafted += nd
    assert drafted > 0 or L < 17                                                    # (the test's own sanity: the longer histories do produce drafts)


def test_scripted_draft_against_the_reference(dev, table):
    from exllamav3_amd import sampling
    rng = np.random.default_rng(5)
    hist = rng.integers(0, VOCAB, MAX_CTX)
    script = rng.integers(0, VOCAB, MAX_CTX)
    script[40] = -1; script[52] = VOCAB; script[61:64] = -1
    sc = torch.as_tensor(script, dtype=I32).to(dev)
    for L in (1, 37, 38, 39, 40, 41, 50, 51, 60, 64, MAX_CTX - 16):
        for k, m in ((1, 2), (3, 4), (3, 6), (15, 16)):
            d = Dev(dev, m, 64)
            _set(d.hist, hist)
            st = np.zeros(R.STATE_WORDS, dtype=np.int64); st[R.BASE], st[R.LIVE] = L - 1, 1
            _set(d.state, st)
            sampling.spec_draft(d.hist, d.state, d.in_tokens, table, d.x0, d.pos, d.seq, d.lens, k, 64, script=sc)
            toks, nd, pos, lens = R.feed(hist, st, m, k, 64, VOCAB, script=script)
            got = d.snapshot()
            assert got["in_tokens"].tolist() == toks and int(got["state"][R.NDRAFT]) == nd, (L, k, m)
            assert got["pos"].tolist() == pos and got["lens"].tolist() == lens
            assert torch.equal(got["x0"].view(torch.int16), table[torch.tensor(toks, device=dev)].cpu().view(torch.int16))


def test_draft_refuses_a_base_whose_rows_would_leave_the_cache(dev, table):
    from exllamav3_amd import sampling
    d = Dev(dev, 4, 64, max_ctx=128)
    _set(d.hist, np.arange(128) % 5)
    st = np.zeros(R.STATE_WORDS, dtype=np.int64); st[R.BASE], st[R.LIVE] = 125, 1       # rows at 125 .. 128: the last one lies outside
    _set(d.state, st)
    before = d.snapshot()
    sampling.spec_draft(d.hist, d.state, d.in_tokens, table, d.x0, d.pos, d.seq, d.lens, 3, 64)
    got = d.snapshot()
    assert int(got["state"][R.INVALID]) == 1 and int(got["state"][R.LIVE]) == 0
    for k in ("in_tokens", "x0", "pos", "seq", "lens", "hist"):
        assert torch.equal(got[k], before[k]), k
    st[R.BASE] = 124                                                                    # 124 .. 127 fit
    _set(d.state, st)
    sampling.spec_draft(d.hist, d.state, d.in_tokens, table, d.x0, d.pos, d.seq, d.lens, 3, 64)
    assert d.pos.tolist() == [124, 125, 126, 127] and int(d.state[R.INVALID]) == 0


ACCEPT_CASES = [
    # name, sampled, in_tokens, n_draft, produced, max_new, stop ids
    ("accept none", [20, 21, 22, 23], [10, 11, 12, 13], 3, 0, 16, ()),
    ("accept two of three", [11, 12, 99, 50], [10, 11, 12, 13], 3, 0, 16, ()),
    ("accept all", [11, 12, 13, 14], [10, 11, 12, 13], 3, 0, 16, ()),
    ("padding is no draft", [11, 10, 10, 10], [10, 11, 10, 10], 1, 0, 16, ()),
    ("no drafts", [11, 12, 13, 14], [10, 10, 10, 10], 0, 3, 16, ()),
    ("stop id in the middle", [11, 12, 13, 14], [10, 11, 12, 13], 3, 0, 16, (12, 500)),
    ("stop id as the token behind the accepted run", [11, 12, 77, 14], [10, 11, 12, 13], 3, 0, 16, (77,)),
    ("stop id only among the rejected", [11, 99, 13, 14], [10, 11, 12, 13], 3, 0, 16, (13, 14)),
    ("budget cut on the last round", [11, 12, 13, 14], [10, 11, 12, 13], 3, 8, 10, ()),
    ("budget of exactly one", [11, 12, 13, 14], [10, 11, 12, 13], 3, 9, 10, ()),
    ("consumed -1 sample", [11, -1, 13, 14], [10, 11, 12, 13], 3, 0, 16, ()),
    ("first sample outside the vocabulary", [VOCAB, 0, 0, 0], [10, 11, 12, 13], 3, 0, 16, ()),
    ("unconsumed -1 samples", [20, -1, -1, -1], [10, 11, 12, 13], 3, 0, 16, ()),
]


@pytest.mark.parametrize("case", ACCEPT_CASES, ids=[c[0] for c in ACCEPT_CASES])
def test_accept_against_the_reference_and_frozen_state_is_idempotent(dev, table, case):
    from exllamav3_amd import sampling
    _, sampled, in_tokens, nd, produced, max_new, stop = case
    d = Dev(dev, 4, max_new, max_ctx=64)
    hist = np.full(64, -1); hist[:5] = [1, 2, 3, 4, 10]
    st = np.zeros(R.STATE_WORDS, dtype=np.int64); st[R.BASE], st[R.PRODUCED], st[R.NDRAFT], st[R.LIVE] = 4, produced, nd, 1
    st[R.ROUNDS], st[R.DRAFTED], st[R.ACCEPTED] = 5, 9, 3
    _set(d.hist, hist); _set(d.state, st); _set(d.sampled, sampled); _set(d.in_tokens, in_tokens); d.round.fill_(6)
    stop_t = torch.tensor(stop, dtype=I32, device=dev) if stop else None
    sampling.spec_accept(d.sampled, d.in_tokens, d.state, d.round, d.hist, d.tokens_out, VOCAB, stop_ids=stop_t, max_new=max_new)
    e_state, e_round, e_hist, e_out = R.accept(sampled, in_tokens, st, 6, hist, np.full(max(max_new, 1), -1), max_new, VOCAB, stop)
    got = d.snapshot()
    assert got["state"].tolist() == e_state.tolist(), (got["state"].tolist(), e_state.tolist())
    assert int(got["round"]) == e_round and got["hist"].tolist() == e_hist.tolist() and got["tokens_out"].tolist() == e_out.tolist()
    if not e_state[R.LIVE]:
        # frozen: three more rounds (accept + draft, then the folded launch) change nothing but the round word
        _set(d.sampled, [5, 6, 7, 8])
        sampling.spec_draft(d.hist, d.state, d.in_tokens, table, d.x0, d.pos, d.seq, d.lens, 3, max_new)
        sampling.spec_accept(d.sampled, d.in_tokens, d.state, d.round, d.hist, d.tokens_out, VOCAB, stop_ids=stop_t, max_new=max_new)
        for _ in range(2):
            sampling.spec_round(d.sampled, d.in_tokens, d.state, d.round, d.hist, d.tokens_out, table, d.x0, d.pos, d.seq, d.lens, 3, stop_ids=stop_t, max_new=max_new)
        again = d.snapshot()
        assert int(again["round"]) == e_round + 3
        for k in ("hist", "state", "in_tokens", "tokens_out", "x0", "pos", "seq", "lens"):
            assert torch.equal(again[k], got[k]), k


@pytest.mark.parametrize("fold", [True, False], ids=["one launch", "two launches"])
@pytest.mark.parametrize("drafter", ["ngram", "script"])
def test_whole_rounds_against_the_reference_with_a_toy_target(dev, table, fold, drafter):
    """A toy target whose token depends on the previous token alone (a map with short cycles, so the n-gram drafter finds repeats; the scripted variant also
    plants one stop token by position): every round the host 'samples' row i as target(in_tokens[i]); the device state is compared with the reference round
    by round, and the output with the target's own sequence."""
    from exllamav3_amd import sampling
    rng = np.random.default_rng(3)
    nxt = rng.integers(0, 12, VOCAB)                                               # everything falls into a cycle among 12 tokens
    prompt, max_new, k, m = [700, 701, 702], 60, 4, 6
    stop = (999,) if drafter == "script" else ()

    def target(tok, position):                                                     # the token AT `position`, behind `tok`
        return 999 if (stop and position == 45) else int(nxt[tok])

    truth = [prompt[-1]]
    for j in range(max_new):
        truth.append(target(truth[-1], 3 + j))
    truth = truth[1:]
    script = None
    if drafter == "script":
        script = np.full(256, -1)
        script[3:3 + max_new] = truth
        script[10] = (script[10] + 1) % 12; script[20:23] = -1; script[31] = (script[31] + 5) % 12     # wrong, absent and wrong again
    sc = torch.as_tensor(script, dtype=I32).to(dev) if script is not None else None
    stop_t = torch.tensor(stop, dtype=I32, device=dev) if stop else None
    d = Dev(dev, m, max_new, max_ctx=256)
    hist = np.full(256, -1); hist[:3] = prompt
    st = np.zeros(R.STATE_WORDS, dtype=np.int64); st[R.BASE], st[R.LIVE] = 2, 1
    _set(d.hist, hist); _set(d.state, st)
    sampling.spec_draft(d.hist, d.state, d.in_tokens, table, d.x0, d.pos, d.seq, d.lens, k, max_new, script=sc)
    out, rnd = np.full(max_new, -1), 0
    for _ in range(max_new + 2):
        f = R.feed(hist, st, m, k, max_new, VOCAB, script=script)
        if f is not None:
            toks = f[0]; st[R.NDRAFT] = f[1]
            assert d.in_tokens.tolist() == toks and d.pos.tolist() == f[2] and d.lens.tolist() == f[3]
            assert torch.equal(d.x0.view(torch.int16), table[torch.tensor(toks, device=dev)].view(torch.int16))
            sampled = [target(t, p + 1) for t, p in zip(toks, f[2])]
        _set(d.sampled, sampled)
        if fold:
            sampling.spec_round(d.sampled, d.in_tokens, d.state, d.round, d.hist, d.tokens_out, table, d.x0, d.pos, d.seq, d.lens, k, script=sc, stop_ids=stop_t)
        else:
            sampling.spec_accept(d.sampled, d.in_tokens, d.state, d.round, d.hist, d.tokens_out, VOCAB, stop_ids=stop_t)
            sampling.spec_draft(d.hist, d.state, d.in_tokens, table, d.x0, d.pos, d.seq, d.lens, k, max_new, script=sc)
        st, rnd, hist, out = R.accept(sampled, toks, st, rnd, hist, out, max_new, VOCAB, stop)
        f = R.feed(hist, st, m, k, max_new, VOCAB, script=script)
        exp = st.copy()
        if f is not None:
            exp[R.NDRAFT] = f[1]
        assert d.state.tolist() == exp.tolist() and int(d.round) == rnd
        assert d.hist.tolist() == hist.tolist() and d.tokens_out.tolist() == out.tolist()
    n = int(st[R.PRODUCED])
    assert not st[R.LIVE] and out[:n].tolist() == truth[:n]
    assert n == (truth.index(stop[0]) + 1 if stop else max_new)
    assert st[R.ACCEPTED] + st[R.ROUNDS] == n and st[R.ACCEPTED] > 0 and st[R.ROUNDS] < rnd
