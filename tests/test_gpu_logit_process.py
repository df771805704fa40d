"""exl3_logit_process (exllamav3_amd.sampling.process_logits, csrc/exl3_logit_process.hip) and exl3_gen_feed_stop on the GPU.  Every logit comparison is bit for
bit against the numpy restatement of the contract (tests/_logit_proc_ref.py); a NaN stands for any NaN."""
import itertools
import numpy as np
import pytest
import torch
import _logit_proc_ref as LP

pytestmark = pytest.mark.gpu

V = 128256
SHAPES = [(V, V), (V, V + 64), (1000, 1008)]                                       # (size, ld)
REPS = [(1.3, 16, 8), (1.1, 10 ** 8, 0), (1.5, 100, 200), (1.2, 0, 64)]
PFS = [(0.4, 0.3, 10 ** 8, 0), (0.0, 0.2, 50, 30), (0.7, 0.0, 5, 0), (0.25, 0.05, 1000, 4000)]
NP = {torch.half: np.float16, torch.float: np.float32}


def _logits(rng, m, size, ld):
    """N(0, 4) in fp16 with fp16 subnormals, +-0, -inf entries and one NaN (row 0)."""
    x = (rng.standard_normal((m, ld)) * 2.0).astype(np.float16)
    for r in range(m):
        idx = rng.integers(0, size, 64)
        x[r, idx[:16]] = -np.inf
        x[r, idx[16:32]] = (rng.integers(1, 1024, 16).astype(np.uint16) | (rng.integers(0, 2, 16).astype(np.uint16) << 15)).view(np.float16)   # subnormals
        x[r, idx[32:40]] = 0.0
        x[r, idx[40:48]] = -0.0
    x[0, int(rng.integers(0, size))] = np.nan
    return x


def _history(rng, kind, m, size):
    """Per row: ids, oldest first.  'long': 5000 ids with heavy repeats (drawn from 64 values) and some ids outside the vocabulary."""
    if kind == "empty":
        return [np.zeros((0,), dtype=np.int32) for _ in range(m)]
    if kind == "one":
        return [rng.integers(0, size, 1).astype(np.int32) for _ in range(m)]
    out = []
    for _ in range(m):
        pool = rng.integers(0, size, 64)
        h = pool[rng.integers(0, 64, 5000)]
        bad = rng.integers(0, 5000, 100)
        h[bad] = rng.choice(np.array([-1, -7, size, size + 3, 2 ** 31 - 1, -2 ** 31]), 100)
        out.append(h.astype(np.int32))
    return out


def _segments(pasts, len_a, cap_b, dev):
    """The histories as the two device segments: past_a [m, len_a], past_b [m, cap_b] (filled with a poison id behind the valid part) and the host len_b."""
    m, n = len(pasts), len(pasts[0])
    len_a = min(len_a, n)
    a = np.stack([p[:len_a] for p in pasts]).astype(np.int32).reshape(m, len_a)
    b = np.full((m, cap_b), 7, dtype=np.int32)
    for r, p in enumerate(pasts):
        b[r, :n - len_a] = p[len_a:]
    return (torch.from_numpy(a).to(dev) if len_a else None), torch.from_numpy(b).to(dev), n - len_a


def _bias(rng, size):
    ids = rng.integers(0, size, 200)
    d = {int(t): float(v) for t, v in zip(ids, rng.standard_normal(200) * 3.0)}
    d[int(ids[0])] = float("-inf")
    return d, [int(t) for t in rng.integers(0, size, 20)] + [size + 5, -3]


def _bitmask(rng, rows, size):
    words = (size + 31) // 32 - 5                                                     # narrower than the vocabulary: the tail is cut
    return rng.integers(0, 2 ** 32, (rows, words), dtype=np.uint64).astype(np.uint32)


def _run(dev, rng, m, size, ld, in_dt, out_dt, hist, use_rep, use_pf, use_bias, bm_rows, inplace, k=0):
    from exllamav3_amd import sampling
    x16 = _logits(rng, m, size, ld)
    x = x16.astype(NP[in_dt])
    pasts = _history(rng, hist, m, size)
    rep = REPS[k % len(REPS)] if use_rep else None
    pf = PFS[k % len(PFS)] if use_pf else None
    bias_d, bans = _bias(rng, size) if use_bias else (None, None)
    bm = _bitmask(rng, m if bm_rows == "per_row" else 1, size) if bm_rows else None
    kw = {}
    if rep:
        kw.update(rep_p=rep[0], rep_sustain=rep[1], rep_decay=rep[2])
    if pf:
        kw.update(pres_p=pf[0], freq_p=pf[1], pf_sustain=pf[2], pf_decay=pf[3])
    procs = sampling.LogitProcessors(logit_bias=bias_d, ban_token_ids=bans, bitmask=None if bm is None else torch.from_numpy(bm.view(np.int32)).to(dev), **kw)
    pa, pb, len_b = _segments(pasts, 3, len(pasts[0]) + 11, dev)
    t_in = torch.from_numpy(x).to(dev)
    t_out = t_in if inplace else torch.full((m, ld), 123.0, dtype=out_dt, device=dev)
    got = sampling.process_logits(t_in, procs, pa, pb, len_b=len_b, size=size, out=t_out)
    assert got is t_out
    bias_vec = None
    if use_bias:
        bias_vec = np.zeros((size,), dtype=np.float32)
        for t, v in procs.bias.items():
            if 0 <= t < size:
                bias_vec[t] = v
    exp = LP.process(x, size, pasts, rep, pf, bias_vec, bm, NP[out_dt])
    g = got.cpu().numpy()
    assert LP.same_bits(g, exp), (m, size, ld, in_dt, out_dt, hist, use_rep, use_pf, use_bias, bm_rows, inplace,
                                  int((g.view(np.uint16 if out_dt == torch.half else np.uint32) != exp.view(np.uint16 if out_dt == torch.half else np.uint32)).sum()))
    return x, exp


def test_every_combination_of_processors(dev):
    """{rep, pres / freq, bias, bitmask (none, shared row, per row)}: all 24 combinations, the other dimensions cycling underneath."""
    rng = np.random.default_rng(11)
    others = itertools.cycle(itertools.product((1, 3, 16), SHAPES, ((torch.half, torch.half), (torch.float, torch.half), (torch.half, torch.float),
                                                                       (torch.float, torch.float)), ("long", "one", "empty", "long")))
    for k, (use_rep, use_pf, use_bias, bm_rows) in enumerate(itertools.product((False, True), (False, True), (False, True), (None, "shared", "per_row"))):
        for _ in range(5):                                                            # (5 and the cycle's 144 are coprime: the combinations drift across it)
            m, (size, ld), (in_dt, out_dt), hist = next(others)
            _run(dev, rng, m, size, ld, in_dt, out_dt, hist, use_rep, use_pf, use_bias, bm_rows, inplace=(in_dt == out_dt and k % 2 == 0), k=k)


@pytest.mark.parametrize("m", [1, 3, 16])
def test_rows_shapes_types_and_histories_with_everything_on(dev, m):
    rng = np.random.default_rng(100 + m)
    k = 0
    for (size, ld), (in_dt, out_dt), hist in itertools.product(SHAPES, itertools.product((torch.half, torch.float), repeat=2), ("empty", "one", "long")):
        for inplace in ((False, True) if in_dt == out_dt else (False,)):
            _run(dev, rng, m, size, ld, in_dt, out_dt, hist, True, True, True, "per_row" if k % 2 else "shared", inplace, k=k)
            k += 1


def test_identity_and_padding_columns(dev):
    """Nothing switched on: the valid columns keep their bits (NaN included), the padding behind `size` is written -inf."""
    from exllamav3_amd import sampling
    rng = np.random.default_rng(5)
    x = _logits(rng, 3, 1000, 1008)
    t = torch.from_numpy(x).to(dev)
    out = sampling.process_logits(t, sampling.LogitProcessors(), size=1000)
    g = out.cpu().numpy()
    assert LP.same_bits(g[:, :1000], x[:, :1000]) and np.isneginf(g[:, 1000:]).all()
    f = sampling.process_logits(t, sampling.LogitProcessors(), size=1000, out=torch.empty((3, 1008), dtype=torch.float, device=dev)).cpu().numpy()
    assert LP.same_bits(f[:, :1000], x[:, :1000].astype(np.float32)) and np.isneginf(f[:, 1000:]).all()


def test_device_length_equals_host_length(dev):
    from exllamav3_amd import sampling
    rng = np.random.default_rng(6)
    m, size, ld = 3, V, V
    x = _logits(rng, m, size, ld)
    pasts = _history(rng, "long", m, size)
    procs = sampling.LogitProcessors(rep_p=1.25, rep_sustain=300, rep_decay=500, pres_p=0.2, freq_p=0.1, pf_sustain=2000, pf_decay=100)
    pa, pb, len_b = _segments(pasts, 1, 6000, dev)
    t = torch.from_numpy(x).to(dev)
    host = sampling.process_logits(t, procs, pa, pb, len_b=len_b, size=size).cpu().numpy()
    for word, bias in ((len_b, 0), (len_b - 40, 40), (len_b + 9, -9)):
        step = torch.tensor([word], dtype=torch.int64, device=dev)
        got = sampling.process_logits(t, procs, pa, pb, step=step, len_b_bias=bias, size=size).cpu().numpy()
        assert LP.same_bits(got, host), (word, bias)
    exp = LP.process(x, size, pasts, (1.25, 300, 500), (0.2, 0.1, 2000, 100), None, None, np.float16)
    assert LP.same_bits(host, exp)
    # the clamp: a word below 0 is an empty second segment, a word past the capacity is the whole of it
    full = [np.concatenate([p[:1], pb[r].cpu().numpy()]) for r, p in enumerate(pasts)]
    for word, hist in ((-5, [p[:1] for p in pasts]), (10 ** 9, full)):
        step = torch.tensor([word], dtype=torch.int64, device=dev)
        got = sampling.process_logits(t, procs, pa, pb, step=step, size=size).cpu().numpy()
        assert LP.same_bits(got, LP.process(x, size, hist, (1.25, 300, 500), (0.2, 0.1, 2000, 100), None, None, np.float16)), word


def test_captured_once_and_replayed_with_the_feed_advancing_the_history(dev):
    """process_logits + gen_feed captured as one graph: the kernel reads the step word and the tokens the feed appended, replay after replay."""
    from exllamav3_amd import sampling
    rng = np.random.default_rng(7)
    m, size, ld, hidden, P, total = 3, 1000, 1008, 64, 3, 12
    embed = torch.from_numpy(rng.standard_normal((size, hidden)).astype(np.float16)).to(dev)
    x0 = torch.zeros((m, hidden), dtype=torch.half, device=dev)
    forced_h = rng.integers(0, 40, (m, P)).astype(np.int32)
    forced = torch.from_numpy(forced_h).to(dev)
    tokens_out = torch.full((m, total), -1, dtype=torch.int32, device=dev)
    sampled = torch.zeros((m,), dtype=torch.int32, device=dev)
    invalid = torch.zeros((m,), dtype=torch.int32, device=dev)
    step = torch.full((1,), -1, dtype=torch.int64, device=dev)
    x = _logits(rng, m, size, ld)
    logits = torch.from_numpy(x).to(dev)
    out = torch.empty_like(logits)
    procs = sampling.LogitProcessors(rep_p=1.4, rep_sustain=2, rep_decay=3, pres_p=0.3, freq_p=0.2, pf_sustain=4, pf_decay=0, ban_token_ids=[5])
    sampling.gen_feed(None, forced, embed, x0, None, None, None, None, invalid, step, vocab=size)            # priming: step word -1 -> 0

    def body():
        sampling.process_logits(logits, procs, forced[:, 0:1], tokens_out, step=step, size=size, out=out)
        sampling.gen_feed(sampled, forced, embed, x0, tokens_out, None, None, None, invalid, step, vocab=size)

    procs.tensors(size, dev)                                                          # (the bias vector is built outside the capture)
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            body()
    torch.cuda.current_stream(dev).wait_stream(st)
    assert int(step) == 0
    hist = [[int(forced_h[r, 0])] for r in range(m)]
    bias = np.zeros((size,), dtype=np.float32)
    bias[5] = -np.inf
    for s in range(8):
        nxt = rng.integers(0, 40, m).astype(np.int32)
        sampled.copy_(torch.from_numpy(nxt))
        graph.replay()
        exp = LP.process(x, size, hist, (1.4, 2, 3), (0.3, 0.2, 4, 0), bias, None, np.float16)
        assert LP.same_bits(out.cpu().numpy(), exp), s
        for r in range(m):
            hist[r].append(int(forced_h[r, s + 1]) if s + 1 < P else int(nxt[r]))
        assert int(step) == s + 1 and tokens_out[:, s].tolist() == [h[-1] for h in hist]


def test_reference_named_ops(dev):
    """ext.apply_rep_pens / apply_pres_freq_pens / apply_logit_bitmask through the reference's argument lists (rep_pen.cu:93, :203; sampling_fused.cu:976)."""
    from exllamav3_amd import ext
    rng = np.random.default_rng(8)
    x = _logits(rng, 1, V, V)
    past = _history(rng, "long", 1, V)
    ids = torch.from_numpy(past[0].astype(np.int64)).view(1, -1).to(dev)
    for dt in (torch.half, torch.float):
        t_in = torch.from_numpy(x.astype(NP[dt])).to(dev)
        out = torch.empty((1, V), dtype=torch.float, device=dev)
        ext.apply_rep_pens(t_in, out, ids, 1.3, 64, 128)
        assert LP.same_bits(out.cpu().numpy(), LP.process(x.astype(NP[dt]), V, past, rep=(1.3, 64, 128), out_dtype=np.float32)), dt
        ext.apply_pres_freq_pens(t_in, out, ids, 0.5, 0.1, 1000, 0)
        assert LP.same_bits(out.cpu().numpy(), LP.process(x.astype(NP[dt]), V, past, pf=(0.5, 0.1, 1000, 0), out_dtype=np.float32)), dt
    # in place on fp32, as the reference's sampler stack calls them (custom.py:778-785); an empty history leaves the logits alone
    t = torch.from_numpy(x.astype(np.float32)).to(dev)
    ext.apply_rep_pens(t, t, ids, 1.2, 10 ** 8, 0)
    ext.apply_pres_freq_pens(t, t, ids, 0.3, 0.2, 10 ** 8, 0)
    step1 = LP.process(x.astype(np.float32), V, past, rep=(1.2, 10 ** 8, 0), out_dtype=np.float32)
    assert LP.same_bits(t.cpu().numpy(), LP.process(step1, V, past, pf=(0.3, 0.2, 10 ** 8, 0), out_dtype=np.float32))
    before = t.clone()
    ext.apply_rep_pens(t, t, torch.zeros((1, 0), dtype=torch.long, device=dev), 1.2, 10 ** 8, 0)
    assert LP.same_bits(t.cpu().numpy(), before.cpu().numpy())
    for bad in (lambda: ext.apply_rep_pens(t, t.half(), ids, 1.2, 10, 0), lambda: ext.apply_rep_pens(t, t, ids.int(), 1.2, 10, 0),
                lambda: ext.apply_pres_freq_pens(t.expand(2, V).contiguous(), t.expand(2, V).contiguous(), ids, 0.1, 0.1, 10, 0)):
        with pytest.raises(RuntimeError):
            bad()
    xb = _logits(rng, 3, V, V)
    for dt, rows in ((torch.half, 1), (torch.float, 3), (torch.half, 3)):
        bm = _bitmask(rng, rows, V)
        t_in = torch.from_numpy(xb.astype(NP[dt])).to(dev)
        out = torch.empty_like(t_in)
        ext.apply_logit_bitmask(t_in, out, torch.from_numpy(bm.view(np.int32)).to(dev))
        assert LP.same_bits(out.cpu().numpy(), LP.process(xb.astype(NP[dt]), V, None, bitmask=bm, out_dtype=NP[dt])), (dt, rows)
    with pytest.raises(RuntimeError):
        ext.apply_logit_bitmask(t_in, out.float(), torch.zeros((1, 8), dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        ext.apply_logit_bitmask(t_in, out, torch.zeros((2, 8), dtype=torch.int32, device=dev))


def test_feed_with_stop_ids(dev):
    from exllamav3_amd import sampling
    rng = np.random.default_rng(9)
    m, size, hidden, total = 3, 1000, 64, 10
    STOP, STOP2, PAD = 17, 23, 17
    embed = torch.from_numpy(rng.standard_normal((size, hidden)).astype(np.float16)).to(dev)
    x0 = torch.zeros((m, hidden), dtype=torch.half, device=dev)
    forced = torch.tensor([[3, STOP, 4], [5, 6, STOP2], [7, 8, 9]], dtype=torch.int32, device=dev)        # stop ids inside the prompt
    tokens_out = torch.full((m, total), -1, dtype=torch.int32, device=dev)
    sampled = torch.zeros((m,), dtype=torch.int32, device=dev)
    cnt = [torch.full((m,), v, dtype=torch.int32, device=dev) for v in (-1, -1, 0)]
    invalid, done = torch.zeros((m,), dtype=torch.int32, device=dev), torch.zeros((m,), dtype=torch.int32, device=dev)
    live = torch.full((1,), -9, dtype=torch.int32, device=dev)
    step = torch.full((1,), -1, dtype=torch.int64, device=dev)
    stop_ids = torch.tensor([STOP, STOP2], dtype=torch.int32, device=dev)

    def feed(tokens, out=tokens_out):
        if tokens is not None:
            sampled.copy_(torch.tensor(tokens, dtype=torch.int32))
        sampling.gen_feed(sampled if tokens is not None else None, forced, embed, x0, out, cnt[0], cnt[1], cnt[2], invalid, step, vocab=size,
                          stop_ids=stop_ids, done=done, pad_token=PAD, live=live)

    def row(t):
        return embed[t].view(torch.int16)

    feed(None, out=None)                                                              # priming
    assert int(step) == 0 and int(live) == 3 and cnt[0].tolist() == [0, 0, 0]
    feed([STOP, STOP, STOP])                                                          # forced tokens win, and a forced stop id does not stop
    feed([STOP, STOP, STOP])
    assert tokens_out[:, :2].tolist() == [[STOP, 4], [6, STOP2], [8, 9]] and done.tolist() == [0, 0, 0] and int(live) == 3
    assert cnt[0].tolist() == [2, 2, 2] and cnt[2].tolist() == [3, 3, 3] and torch.equal(x0[1].view(torch.int16), row(STOP2))
    feed([11, STOP2, 12])                                                             # row 1 samples a stop id: recorded, not fed
    assert tokens_out[:, 2].tolist() == [11, STOP2, 12] and done.tolist() == [0, 1, 0] and int(live) == 2
    assert cnt[0].tolist() == [3, 2, 3] and cnt[1].tolist() == [3, 2, 3] and cnt[2].tolist() == [4, 3, 4]
    assert torch.equal(x0[1].view(torch.int16), row(STOP2)) and torch.equal(x0[0].view(torch.int16), row(11)) and torch.equal(x0[2].view(torch.int16), row(12))
    x1 = x0[1].clone()
    feed([13, 14, -1])                                                                # the done row: pad, frozen; row 2 goes invalid and leaves `live` too
    assert tokens_out[:, 3].tolist() == [13, PAD, -1] and done.tolist() == [0, 1, 0] and invalid.tolist() == [0, 0, 1] and int(live) == 1
    assert cnt[0].tolist() == [4, 2, 4] and torch.equal(x0[1], x1) and torch.equal(x0[2].view(torch.int16), row(12))
    feed([STOP, 15, 16])                                                              # the last live row stops
    assert tokens_out[:, 4].tolist() == [STOP, PAD, -1] and done.tolist() == [1, 1, 0] and int(live) == 0
    assert cnt[0].tolist() == [4, 2, 5] and torch.equal(x0[0].view(torch.int16), row(13)) and torch.equal(x0[1], x1)
    feed([1, 2, 3])
    assert tokens_out[:, 5].tolist() == [PAD, PAD, -1] and int(live) == 0 and int(step) == 6 and cnt[0].tolist() == [4, 2, 6] and cnt[2].tolist() == [5, 3, 7]
    assert (tokens_out[:, 6:] == -1).all()
    # without the stop arguments the entry is exl3_gen_feed: `done` is not consulted
    sampling.gen_feed(sampled, forced, embed, x0, tokens_out, cnt[0], cnt[1], cnt[2], invalid, step, vocab=size)
    assert tokens_out[:, 6].tolist() == [1, 2, -1] and cnt[0].tolist() == [5, 3, 7]
    with pytest.raises(RuntimeError):
        sampling.gen_feed(sampled, forced, embed, x0, tokens_out, cnt[0], cnt[1], cnt[2], invalid, step, vocab=size, stop_ids=stop_ids)
