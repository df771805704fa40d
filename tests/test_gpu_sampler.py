"""The device sampler (exllamav3_amd.sampling.sample -> exl3_sample, csrc/exl3_sampler.hip) against the CPU restatement of its contract (tests/_sampler_ref.py):
full vocabulary (128 256 columns), a padded case (size < ld with large values, NaN and +Inf planted in the padding), m in {1, 3, 16}.
Integers (greedy token, top-k cutoff and kept count, min-p threshold) are compared for equality; top-p and the sampled token by the derived bars below."""
import math
import numpy as np
import pytest
import torch
import _sampler_ref as R

pytestmark = pytest.mark.gpu

V = 128256
SHAPES = [(V, V), (V, 128000)]                 # (ld, size)
MS = [1, 3, 16]

#: top-p: relative mass perturbation under which the GPU's cutoff must be a valid answer.  The kernel sums 2^40 fixed-point masses of expf((l - M) * itf):
#: expf's relative error including the rounding of its fp32 argument <= 2^-21 (4.8e-7), the conversion to fixed point truncates < 1 unit per element against
#: Z >= 2^40 (the top element weighs 1): <= V * 2^-40 = 1.2e-7, the target p * Z is formed in fp64 and floored (< 1 unit); the sums themselves are integer: exact.
TOPP_EPS = 1e-6


def _rows(m, ld, size, seed, coarse=False):
    """fp16 [m, ld]: sigma 3, every second row with five planted +8 peaks; `coarse`: quarter steps (many exact ties).  Padding: large values, a NaN, a +Inf."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, ld)) * 3.0
    for r in range(0, m, 2):
        x[r, rng.choice(size, 5, replace=False)] += 8.0
    if coarse:
        x = np.round(x * 4) / 4
    x = x.astype(np.float16)
    if size < ld:
        x[:, size:] = 60000.0
        x[:, size + 1] = np.nan
        x[:, size + 2] = np.inf
    return x


def _run(dev, x, size, mode, step=0, seed=0, row0=0, **kw):
    from exllamav3_amd import sampling
    ka = sampling.KernelArgs(mode, kw.get("filters", 0), kw.get("top_k", 0), kw.get("top_p", 1.0), kw.get("inv_temp", 1.0), kw.get("inv_temp_filter", 1.0),
                             kw.get("minp_log", 0.0), seed)
    t = torch.from_numpy(x).to(dev)
    m = x.shape[0]
    stepw = torch.tensor([step], dtype=torch.int64, device=dev)
    cut = torch.empty((m,), dtype=torch.float, device=dev)
    kept = torch.empty((m,), dtype=torch.int32, device=dev)
    ws = sampling.workspace(m, dev)
    tok = sampling.sample(t, ka, stepw, size=size, row0=row0, ws=ws, cutoff_out=cut, kept_out=kept)
    torch.cuda.synchronize()
    raw = ws.cpu().numpy().view(np.float32).reshape(m, -1)[:, 0].copy()          # word 0 of a row's workspace: the cutoff the select kernel decided (modes 2 / 3)
    assert not ws.cpu().numpy().view(np.uint32).reshape(m, -1)[:, 2].any(), "the ticket words must be left zeroed"
    return tok.cpu().numpy(), cut.cpu().numpy(), kept.cpu().numpy(), raw


@pytest.mark.parametrize("ld,size", SHAPES)
@pytest.mark.parametrize("m", MS)
def test_greedy_is_the_lowest_index_argmax(dev, m, ld, size):
    x = _rows(m, ld, size, 100 + m)
    x[0, :size] = np.random.default_rng(1).integers(-1, 2, size).astype(np.float16)      # few distinct values: thousands of equal maxima
    if m > 1:
        # exact ties planted across the column ranges of the pick kernel's workgroups (2040 columns each) and far apart
        x[1, :size] = np.minimum(x[1, :size], np.float16(9.0))
        for i in (2039, 2040, 50000, 100000, size - 1):
            x[1, i] = 11.0
        x[2, :size] = -np.abs(x[2, :size]) - np.float16(1.0)
        x[2, 4000], x[2, 300] = 0.0, -0.0                                                 # -0 == +0: index 300 wins
    tok, cut, kept, _ = _run(dev, x, size, 0)
    exp = np.array([R.greedy(x[r, :size]) for r in range(m)])
    assert np.array_equal(tok, exp), (tok, exp)
    if m > 1:
        assert tok[1] == 2039 and tok[2] == 300


@pytest.mark.parametrize("ld,size", SHAPES)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", [1, 8, 50, 1000])
def test_topk_cutoff_and_kept_count_are_exact(dev, m, ld, size, k):
    x = _rows(m, ld, size, 200 + m + k, coarse=True)                                      # quarter steps: ties at every cutoff
    tok, cut, kept, raw = _run(dev, x, size, 3, filters=1, top_k=k, step=3, seed=11)
    for r in range(m):
        l = x[r, :size]
        c = R.topk_cutoff(l, k)
        n = int((l.astype(np.float64) >= c).sum())
        assert n >= k and (cut[r], raw[r], kept[r]) == (c, c, n), (r, cut[r], raw[r], kept[r], c, n)
        assert l[tok[r]] >= c


@pytest.mark.parametrize("ld,size", SHAPES)
@pytest.mark.parametrize("m", MS)
def test_minp_threshold_is_one_fp32_add(dev, m, ld, size):
    x = _rows(m, ld, size, 300 + m)
    for mode, kw in ((2, {}), (3, {"filters": 4})):
        for min_p in (0.5, 0.05, 1e-3):
            tok, cut, kept, raw = _run(dev, x, size, mode, minp_log=math.log(min_p), step=1, seed=5, **kw)
            for r in range(m):
                l = x[r, :size].astype(np.float64)
                thr = R.minp_threshold(x[r, :size], np.float32(math.log(min_p)))
                assert raw[r] == np.float32(thr)
                assert kept[r] == int((l >= thr).sum()) and cut[r] == l[l >= thr].min() and l[tok[r]] >= thr


def _topp_ok(l, c, c0, p, itf):
    """The criterion: mass(l >= c) <= p Z (1 + eps) unless c is the top class, and mass(l >= next value below c) > p Z (1 - eps)."""
    vals, w, Z = R.masses(l, c0, itf)
    assert c in vals, "the cutoff must be a surviving value"
    i = int(np.nonzero(vals == c)[0][0])
    cum = np.cumsum(w)
    p = float(np.float32(p))
    ok_hi = i == 0 or cum[i] <= p * Z * (1 + TOPP_EPS)
    ok_lo = i + 1 == vals.size or cum[i + 1] > p * Z * (1 - TOPP_EPS)
    return ok_hi and ok_lo, (cum[i] / Z, cum[min(i + 1, vals.size - 1)] / Z, p)


@pytest.mark.parametrize("ld,size", SHAPES)
@pytest.mark.parametrize("m", MS)
def test_topp_cutoff_is_valid_within_the_derived_mass_perturbation(dev, m, ld, size):
    for ci, (filters, k, p, itf, min_p) in enumerate([(2, 0, 0.9, 1.0, 0), (2, 0, 0.5, 1.25, 0), (2, 0, 0.95, 0.5, 0), (3, 50, 0.9, 1.25, 0), (3, 1000, 0.6, 1.0, 0),
                                                       (6, 0, 0.9, 1.0, 0.01), (7, 50, 0.9, 1.25, 0.02), (2, 0, 1.0, 1.0, 0), (2, 0, 1e-4, 1.0, 0)]):
        x = _rows(m, ld, size, 400 + m + 10 * ci, coarse=(ci % 2 == 1))
        mpl = np.float32(math.log(min_p)) if min_p else np.float32(0.0)
        tok, cut, kept, raw = _run(dev, x, size, 3, filters=filters, top_k=k, top_p=p, inv_temp_filter=itf, minp_log=float(mpl), step=2, seed=3)
        for r in range(m):
            l = x[r, :size]
            c0 = R.cutoff(l, 3, filters=filters & 5, top_k=k, minp_log=mpl)
            ok, info = _topp_ok(l, float(cut[r]), c0, p, itf)
            assert ok, (ci, r, info)
            assert kept[r] == int((l.astype(np.float64) >= cut[r]).sum()) and l[tok[r]] >= cut[r]


def _token_cases():
    cases = []
    for it in (0.5, 1.0, 1.25, 2.0):
        cases += [(1, dict(inv_temp=it)), (2, dict(inv_temp=it, minp_log=float(np.float32(math.log(0.05))))),
                  (3, dict(inv_temp=it, filters=3, top_k=50, top_p=0.9, inv_temp_filter=it)),
                  (3, dict(inv_temp=it, filters=7, top_k=1000, top_p=0.95, inv_temp_filter=1.0, minp_log=float(np.float32(math.log(0.01)))))]
    return cases


def _check_tokens(x, size, tok, mode, kw, step, seed, row0, dev_stats):
    for r in range(x.shape[0]):
        l = x[r, :size]
        cutkw = {a: kw[a] for a in ("filters", "top_k", "top_p", "inv_temp_filter", "minp_log") if a in kw}
        v = R.objective(l, kw["inv_temp"], row0 + r, step, seed, R.cutoff(l, mode, **cutkw))
        tol = 16 * 2.0 ** -24 * np.abs(v[np.isfinite(v)]).max()
        dev_stats["rows"] += 1
        dev_stats["differ"] += int(tok[r] != int(np.argmax(v)))
        dev_stats["max_dev"] = max(dev_stats["max_dev"], float(v.max() - v[tok[r]]) if tok[r] >= 0 else np.inf)
        assert tok[r] >= 0 and v[tok[r]] >= v.max() - tol, (mode, kw, r, int(tok[r]), int(np.argmax(v)), float(v.max() - v[tok[r]]), tol)


def test_sampled_tokens_maximise_the_objective(dev):
    """Modes 1-3: with the restatement's objective v (fp64) over the restatement's kept set, the GPU's token t satisfies v[t] >= max(v) - 16 * 2^-24 * max|v| (the fp32
    evaluation of one product, two logs, one add), and differs from the restatement's own argmax in at most 1 % of the rows."""
    stats = {"rows": 0, "differ": 0, "max_dev": 0.0}
    for ci, (mode, kw) in enumerate(_token_cases()):
        for m, (ld, size) in ((16, SHAPES[ci % 2]), (3, SHAPES[(ci + 1) % 2]), (1, SHAPES[ci % 2])):
            x = _rows(m, ld, size, 500 + 7 * ci + m)
            step, seed = 1000 + ci, (ci << 33) | 77
            tok, _, _, _ = _run(dev, x, size, mode, step=step, seed=seed, **kw)
            _check_tokens(x, size, tok, mode, kw, step, seed, 0, stats)
    print("sampled tokens:", stats)
    assert stats["differ"] <= 0.01 * stats["rows"], f"GPU token != restatement argmax in {stats['differ']} of {stats['rows']} rows (largest objective deviation {stats['max_dev']:.3e})"


def test_noise_is_keyed_by_row_and_step_not_by_the_batch(dev):
    from exllamav3_amd import sampling
    x = _rows(16, V, V, 600)
    kw = dict(inv_temp=1.0, filters=3, top_k=50, top_p=0.9)
    t16, _, _, _ = _run(dev, x, V, 3, step=9, seed=42, **kw)
    for r in (0, 5, 15):
        t1, _, _, _ = _run(dev, x[r:r + 1], V, 3, step=9, seed=42, row0=r, **kw)
        assert t1[0] == t16[r]
    t16b, _, _, _ = _run(dev, x, V, 1, step=9, seed=42)
    t16c, _, _, _ = _run(dev, x, V, 1, step=9, seed=43)
    assert not np.array_equal(t16b, t16c)
    # a replayed graph reads the step word on the device: capture once, bump the word, replay
    ka = sampling.KernelArgs(1, 0, 0, 1.0, 1.0, 1.0, 0.0, 42)
    t = torch.from_numpy(x).to(dev)
    stepw = torch.tensor([9], dtype=torch.int64, device=dev)
    out = torch.empty((16,), dtype=torch.int32, device=dev)
    ws = sampling.workspace(16, dev)
    sampling.sample(t, ka, stepw, out=out, ws=ws)
    st = torch.cuda.Stream(); st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            sampling.sample(t, ka, stepw, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(st)
    g.replay(); torch.cuda.synchronize()
    a = out.cpu().numpy().copy()
    assert np.array_equal(a, t16b)
    stepw += 1
    g.replay(); torch.cuda.synchronize()
    b = out.cpu().numpy().copy()
    assert not np.array_equal(a, b)
    stats = {"rows": 0, "differ": 0, "max_dev": 0.0}
    _check_tokens(x, V, b, 1, dict(inv_temp=1.0), 10, 42, 0, stats)
    stepw -= 1
    g.replay(); torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), a)


@pytest.mark.parametrize("ld,size", SHAPES)
def test_invalid_rows_yield_minus_one_and_minus_inf_is_never_chosen(dev, ld, size):
    x = _rows(16, ld, size, 700)
    x[1, 77] = np.nan
    x[2, size - 1] = np.inf
    x[3, :size] = -np.inf
    x.view(np.uint16)[4, 5] = 0xFE00                                                      # a NaN with the sign bit set
    x[5, :size] = -np.inf
    x[5, [10, 70000, size - 1]] = [-3.0, -2.5, -60000.0]
    x[6, ::2] = -np.inf
    bad = {1, 2, 3, 4}
    for mode, kw in [(0, {}), (1, dict(inv_temp=1.0)), (2, dict(inv_temp=1.0, minp_log=-2.0)), (3, dict(inv_temp=0.7, filters=7, top_k=40, top_p=0.9, minp_log=-3.0)),
                     (3, dict(inv_temp=1.0, filters=1, top_k=1000))]:
        for step in range(3):
            tok, cut, kept, _ = _run(dev, x, size, mode, step=step, seed=8, **kw)
            for r in range(16):
                if r in bad:
                    assert tok[r] == -1 and kept[r] == 0, (mode, r, tok[r])
                else:
                    assert 0 <= tok[r] < size and np.isfinite(x[r, tok[r]]), (mode, r, tok[r])
            assert tok[5] in (10, 70000, size - 1)
            assert tok[6] % 2 == 1
    tok, cut, kept, _ = _run(dev, x, size, 3, inv_temp=1.0, filters=1, top_k=1000, seed=8)
    assert kept[5] == 3 and cut[5] == -60000.0                                            # fewer than k finite values: all of them, never -Inf
