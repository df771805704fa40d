"""The MoE router and expert dispatch at the expert counts of real checkpoints (32 .. 512 experts, top-4 .. top-16, router bias), where the rest of the
suite stays at Mixtral's 8 x top-2: routing_std / routing_std_norm / routing_std_fx (csrc/exl3_routing.hip) against float64 and the oracle's stable
sort, ties and non-finite rows, moe_build_slots / moe_scatter against their restatement (tests/_moe_ref.py), and the indexed launches end to end at
128 experts x top-8 against the oracle's per-assignment composition."""
import numpy as np
import pytest
import torch
from oracle import exl3_oracle as o

import _moe_ref as R

pytestmark = pytest.mark.gpu

EPS = 1e-5
SS_RTOL = 129 * 2.0 ** -24            # a block's sum of 128 squares in fp32, any order: 128 products and 127 additions, each rounding <= 2^-24 of a positive partial sum


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------
# router
# ------------------------------------------------------------------------------------------------

def _route(dev, entry, x, gate, K, bias=None, pes=None, norm_w=None, slots=True):
    """One router launch.  entry "std": x is the fp16 router input; "norm": x is the fp16 residual, the launch normalises it (block sums from
    glue_resid); "fx": the same residual as int64 fixed point.  -> dict of numpy outputs (scores, sel, w, gu, and xn / ss for norm / fx)."""
    from exllamav3_amd import ext
    rows, hidden = x.shape
    E = gate.shape[1]
    sc = torch.full((rows, E), 77.0, dtype=torch.half, device=dev)
    sel = torch.full((rows, K), -7, dtype=torch.long, device=dev)
    wt = torch.full((rows, K), 77.0, dtype=torch.half, device=dev)
    gu = torch.full((2, rows * K), -7, dtype=torch.long, device=dev) if slots else None
    b = None if bias is None else _T(bias, dev)
    out = {}
    if entry == "std":
        ext.routing_std(_T(x, dev), _T(gate, dev), sc, sel, wt, per_expert_scale=pes, bias=b, gu_slots=gu)
    else:
        assert pes is None
        xn = torch.empty((rows, hidden), dtype=torch.half, device=dev)
        ss = torch.full((rows, hidden // 128), float("nan"), dtype=torch.float, device=dev)
        if entry == "norm":
            dx = _T(x, dev)
            ext.glue_resid(None, 0, None, None, dx, ss, rows)                 # per-block sums of squares of x (x itself unchanged)
            ext.routing_std_norm(dx, _T(norm_w, dev), ss, EPS, xn, _T(gate, dev), sc, sel, wt, bias=b, gu_slots=gu)
        else:
            Rfx = _T(np.rint(x.astype(np.float64) * 2.0 ** 32).astype(np.int64), dev)      # fp16(R / 2^32) == x exactly
            ext.routing_std_fx(Rfx, _T(norm_w, dev), ss, EPS, xn, _T(gate, dev), sc, sel, wt, bias=b, gu_slots=gu)
        out["xn"], out["ss"] = _np(xn), _np(ss)
    torch.cuda.synchronize()
    out.update(scores=_np(sc), sel=_np(sel), w=_np(wt), gu=None if gu is None else _np(gu))
    return out


def _logits(scores, bias):
    """The launch's fp32 logits: fp16 score + fp16 bias, one fp32 add."""
    l = scores.astype(np.float32)
    return l if bias is None else (l + bias.astype(np.float32)[None, :]).astype(np.float32)


def _within_one_fp16_ulp(got, want64):
    """got (fp16) is the correctly rounded fp16 of want64 or one of its two neighbours."""
    r = want64.astype(np.float16)
    lo, hi = np.nextafter(r, np.float16(-np.inf)), np.nextafter(r, np.float16(np.inf))
    return (got >= lo) & (got <= hi)


def _check_weights(res, bias, pes=None, rows=None):
    """Weights: one fp16 ulp around the float64 softmax over the launch's own selected logits (x the bf16 scale's value, one rounding).  Derived: the
    fp32 expf, sum and divide err by ~1e-6 relative, far below half an fp16 ulp (4.9e-4) -> the correctly rounded value or its neighbour."""
    sel = res["sel"]
    lg = np.take_along_axis(_logits(res["scores"], bias), sel, axis=-1).astype(np.float64)
    e = np.exp(lg - lg[:, :1])
    want = e / e.sum(-1, keepdims=True)
    if pes is not None:
        want = want * pes.astype(np.float64)[sel]
    ok = _within_one_fp16_ulp(res["w"], want)
    if rows is not None:
        ok = ok[rows]
    assert ok.all(), (res["w"][~ok] if rows is None else None, want.astype(np.float16)[~ok] if rows is None else None)


def _check_selection(res, bias, E, K):
    """Selection == the oracle's routing on the launch's own fp16 scores (a last-ulp score cannot flip a near-tie); K distinct indices in [0, E) in
    non-increasing logit order; gu_slots == [sel | sel + E]."""
    sc, sel = res["scores"], res["sel"]
    assert np.isfinite(sc.astype(np.float32)).all()
    _, sel_ref, _ = o.routing_std(sc, np.eye(E, dtype=np.float16), K, bias=bias)          # scores @ I == scores exactly
    assert np.array_equal(sel, sel_ref)
    assert ((sel >= 0) & (sel < E)).all()
    assert all(len(set(r.tolist())) == K for r in sel)
    lg = np.take_along_axis(_logits(sc, bias), sel, axis=-1)
    assert (np.diff(lg, axis=-1) <= 0).all()
    if res["gu"] is not None:
        assert np.array_equal(res["gu"], np.stack([sel.reshape(-1), sel.reshape(-1) + E]))


def _check_scores(res, x_in, gate):
    ref = x_in.astype(np.float64) @ gate.astype(np.float64)
    assert np.abs(res["scores"].astype(np.float64) - ref).max() < 2e-3 * max(1.0, float(np.abs(ref).max()))


def _same_bits(a, b, keys=("scores", "sel", "w", "gu")):
    return all(np.array_equal(a[k].view(np.uint16) if a[k].dtype == np.float16 else a[k], b[k].view(np.uint16) if b[k].dtype == np.float16 else b[k])
               for k in keys)


ROUTER_CASES = [(2880, 32, 4), (2048, 128, 8), (7168, 256, 8), (7168, 384, 8), (2048, 512, 16), (1024, 160, 6), (512, 16, 16)]


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("hidden,E,K", ROUTER_CASES)
def test_router_at_real_expert_counts(dev, hidden, E, K, rows):
    """routing_std, and for hidden % 128 == 0 routing_std_norm and routing_std_fx, at the (hidden, experts, top-k) of gpt-oss (32 x 4, bias, hidden not
    a multiple of 128), Qwen3-MoE (128 x 8), the 256- and 384-expert models (384 / 8 = 48 does not divide 256: the per-expert loop), the launch's limits
    (512 x 16), a loop-path count (160) and K == E; with and without bias, with gu_slots, the plain entry also with per_expert_scale.  Scores against the
    float64 product, the selection against the oracle on the launch's own scores, the weights to one fp16 ulp; the three entries agree bit for bit on the
    same normalised row."""
    rng = np.random.default_rng([hidden, E, K, rows])
    x = (rng.standard_normal((rows, hidden)) * 2).astype(np.float16)
    gate = (rng.standard_normal((hidden, E)) / np.sqrt(hidden)).astype(np.float16)
    bias = (rng.standard_normal(E) * 0.5).astype(np.float16)
    pes_t = torch.from_numpy(rng.uniform(0.5, 2.0, E).astype(np.float32)).to(torch.bfloat16)
    pes = pes_t.float().numpy()
    for b in (None, bias):
        res = _route(dev, "std", x, gate, K, bias=b)
        _check_scores(res, x, gate)
        _check_selection(res, b, E, K)
        _check_weights(res, b)
        scaled = _route(dev, "std", x, gate, K, bias=b, pes=pes_t.to(dev), slots=False)
        assert _same_bits(res, scaled, ("scores", "sel"))
        _check_weights(scaled, b, pes=pes)
        if hidden % 128:
            continue
        norm_w = (1 + 0.1 * rng.standard_normal(hidden)).astype(np.float16)
        rn = _route(dev, "norm", x, gate, K, bias=b, norm_w=norm_w)
        xn_ref = o.rms_norm(x, norm_w, EPS).astype(np.float32)
        assert np.abs(rn["xn"].astype(np.float32) - xn_ref).max() <= 2e-3 * np.abs(xn_ref).max()
        _check_scores(rn, rn["xn"], gate)
        _check_selection(rn, b, E, K)
        _check_weights(rn, b)
        # the three entry points on the same normalised row: identical bits
        rf = _route(dev, "fx", x, gate, K, bias=b, norm_w=norm_w)
        assert np.array_equal(rf["xn"].view(np.uint16), rn["xn"].view(np.uint16)) and _same_bits(rf, rn)
        assert np.allclose(rf["ss"], rn["ss"], rtol=1e-6)
        rs = _route(dev, "std", rn["xn"], gate, K, bias=b)
        assert _same_bits(rs, rn)


def test_router_rejects_a_bias_of_the_wrong_dtype_length_or_layout(dev):
    """A float32 bias used to be read as float16 pairs; a short one ran past its end."""
    from exllamav3_amd import ext
    rows, hidden, E, K = 2, 256, 32, 4
    x = torch.zeros((rows, hidden), dtype=torch.half, device=dev); gate = torch.zeros((hidden, E), dtype=torch.half, device=dev)
    sc = torch.empty((rows, E), dtype=torch.half, device=dev); sel = torch.empty((rows, K), dtype=torch.long, device=dev)
    wt = torch.empty((rows, K), dtype=torch.half, device=dev)
    w = torch.ones((hidden,), dtype=torch.half, device=dev); ss = torch.ones((rows, hidden // 128), dtype=torch.float, device=dev)
    xn = torch.empty_like(x); Rfx = torch.zeros((rows, hidden), dtype=torch.long, device=dev)
    good = torch.zeros((E,), dtype=torch.half, device=dev)
    bad = [torch.zeros((E,), dtype=torch.float, device=dev), torch.zeros((E,), dtype=torch.bfloat16, device=dev), torch.zeros((E - 1,), dtype=torch.half, device=dev),
           torch.zeros((2 * E,), dtype=torch.half, device=dev), torch.zeros((2 * E,), dtype=torch.half, device=dev)[::2], torch.zeros((E,), dtype=torch.half)]
    calls = [lambda b: ext.routing_std(x, gate, sc, sel, wt, bias=b),
             lambda b: ext.routing_std_norm(x, w, ss, EPS, xn, gate, sc, sel, wt, bias=b),
             lambda b: ext.routing_std_fx(Rfx, w, ss, EPS, xn, gate, sc, sel, wt, bias=b)]
    for call in calls:
        call(good)
        call(None)
        for b in bad:
            with pytest.raises(RuntimeError):
                call(b)
    torch.cuda.synchronize()


@pytest.mark.parametrize("E", [128, 160])
def test_router_ties_go_to_the_lower_index(dev, E):
    """Duplicate gate columns give bit-identical scores on the vector path (E = 128) and the per-expert loop (E = 160): every expert sums the same rows in
    the same order.  Columns 5, 69 and 70 are the top three (5 and 69 are candidates j = 0, 1 of the same lane, 70 sits on another lane): the selection
    begins 5, 69, 70.  A second group of five equal columns straddles the K-th place: its three lowest indices are selected.  Then the same with all
    those scores equal and the groups separated only by equal bias values."""
    hidden, K = 256, 8
    rng = np.random.default_rng(E)
    x = rng.standard_normal((1, hidden)).astype(np.float16)
    xf = x[0].astype(np.float64)
    unit = xf / (xf @ xf)                                                     # x . unit == 1
    top, singles, straddle = [5, 69, 70], [100, 20], [127, 9, 73, 30, 94]
    want = np.array([[5, 69, 70, 100, 20, 9, 30, 73]])
    gate = (rng.standard_normal((hidden, E)) * 0.3 / np.sqrt(hidden)).astype(np.float16)     # the other scores: |s| well below 3
    for cols, s in ((top, 6.0), (singles[:1], 5.0), (singles[1:], 4.5), (straddle, 3.0)):
        gate[:, cols] = (unit * s).astype(np.float16)[:, None]
    res = _route(dev, "std", x, gate, K)
    sc = res["scores"][0]
    assert len(set(sc[top].view(np.uint16).tolist())) == 1 and len(set(sc[straddle].view(np.uint16).tolist())) == 1
    rest = np.setdiff1d(np.arange(E), top + singles + straddle)
    assert sc[top][0] > sc[100] > sc[20] > sc[straddle][0] > sc[rest].max()
    assert np.array_equal(res["sel"], want)
    _check_selection(res, None, E, K)
    _check_weights(res, None)
    # equal scores, equal bias values
    gate[:, top + singles + straddle] = (unit * 2.0).astype(np.float16)[:, None]
    bias = np.zeros(E, dtype=np.float16)
    bias[top], bias[100], bias[20], bias[straddle] = 3.0, 2.0, 1.5, 1.0
    res = _route(dev, "std", x, gate, K, bias=bias)
    sc = res["scores"][0]
    assert len(set(sc[top + singles + straddle].view(np.uint16).tolist())) == 1 and sc[5] + 1.0 > sc[rest].max()
    assert np.array_equal(res["sel"], want)
    _check_selection(res, bias, E, K)
    _check_weights(res, bias)


def _stable_topk(logits, K):
    """The oracle's ranking: stable descending sort -- +inf, finite values, -inf, NaN; ties to the lower index."""
    return np.argsort(-logits, axis=-1, kind="stable")[:, :K]


def _nonfinite_inputs():
    hidden, E, K = 256, 128, 8
    rng = np.random.default_rng(128)
    x = rng.standard_normal((3, hidden)).astype(np.float16)
    gate = (rng.standard_normal((hidden, E)) / np.sqrt(hidden)).astype(np.float16)
    return hidden, E, K, rng, x, gate


def _check_nonfinite_contract(res, bias, E, K):
    sel = res["sel"]
    assert ((sel >= 0) & (sel < E)).all(), sel
    assert all(len(set(r.tolist())) == K for r in sel), sel
    assert np.array_equal(sel, _stable_topk(_logits(res["scores"], bias), K)), sel
    assert np.array_equal(res["gu"], np.stack([sel.reshape(-1), sel.reshape(-1) + E]))


def test_router_row_with_a_nan_hidden_state_selects_experts_0_to_k(dev):
    """A NaN in the hidden state makes every score of the row NaN: the row selects experts 0 .. K - 1 (all logits tie at the bottom rank), the other rows
    come out bit-identical to a launch without the bad row.  Before the fix the row's eight indices were 0x7fffffff."""
    hidden, E, K, rng, x, gate = _nonfinite_inputs()
    good = _route(dev, "std", x, gate, K)
    xb = x.copy(); xb[1, 77] = np.nan
    res = _route(dev, "std", xb, gate, K)
    assert np.isnan(res["scores"][1].astype(np.float32)).all()
    assert res["sel"][1].tolist() == list(range(K)), res["sel"][1]
    _check_nonfinite_contract(res, None, E, K)
    for k in ("scores", "w"):
        assert np.array_equal(res[k][[0, 2]].view(np.uint16), good[k][[0, 2]].view(np.uint16))
    assert np.array_equal(res["sel"][[0, 2]], good["sel"][[0, 2]])


def test_router_row_mixing_both_infinities_and_nan(dev):
    """A +inf in the hidden state of one row: its scores are +inf where the gate entry of that hidden row is positive, -inf where it is negative and NaN
    where it is zero.  The +inf experts come first (by index), then the lowest -inf ones, no NaN one; the other rows are bit-identical to a clean launch."""
    hidden, E, K, rng, x, gate = _nonfinite_inputs()
    h0 = 31
    pos, nan = [90, 17], [0, 1, 2, 40, 64, 127]
    gate[h0] = -np.abs(gate[h0]) - np.float16(0.01)
    gate[h0, pos] = 0.25
    gate[h0, nan] = 0.0
    good = _route(dev, "std", x, gate, K)
    xb = x.copy(); xb[1, h0] = np.inf
    res = _route(dev, "std", xb, gate, K)
    s1 = res["scores"][1].astype(np.float32)
    assert np.isposinf(s1[pos]).all() and np.isnan(s1[nan]).all() and np.isneginf(np.delete(s1, pos + nan)).all()
    assert res["sel"][1].tolist() == [17, 90, 3, 4, 5, 6, 7, 8], res["sel"][1]
    _check_nonfinite_contract(res, None, E, K)
    for k in ("scores", "w"):
        assert np.array_equal(res[k][[0, 2]].view(np.uint16), good[k][[0, 2]].view(np.uint16))
    assert np.array_equal(res["sel"][[0, 2]], good["sel"][[0, 2]])


@pytest.mark.parametrize("case", ["neginf_all_but_5", "nan_on_10", "nan_on_125", "neginf_and_nan"])
def test_router_bias_masks_and_nan_bias_never_leave_the_expert_range(dev, case):
    """Experts masked with a -inf bias, or carrying a NaN bias: the launch still writes K distinct indices in [0, E), ranked as the oracle's stable
    descending sort ranks the logits (finite, then -inf, then NaN; ties to the lower index); the scores (which carry no bias) are bit-identical to a
    launch without bias.  Weights are asserted only where every selected logit is finite.  Before the fix every place past the last logit above -1e30
    held 0x7fffffff."""
    hidden, E, K, rng, x, gate = _nonfinite_inputs()
    bias = (rng.standard_normal(E) * 0.25).astype(np.float16)
    perm = rng.permutation(E)
    if case == "neginf_all_but_5":
        keep = np.sort(perm[:5]); masked = np.sort(perm[5:])
        bias[masked] = -np.inf
    elif case == "nan_on_10":
        nan = perm[:10]
        bias[nan] = np.nan
    elif case == "nan_on_125":
        keep = np.sort(perm[:3]); masked = np.sort(perm[3:])
        bias[masked] = np.nan
    else:
        keep = np.sort(perm[:3]); masked = np.sort(perm[3:103]); nan = perm[103:]
        bias[masked] = -np.inf; bias[nan] = np.nan
    clean = _route(dev, "std", x, gate, K)
    res = _route(dev, "std", x, gate, K, bias=bias)
    assert np.array_equal(res["scores"].view(np.uint16), clean["scores"].view(np.uint16))
    _check_nonfinite_contract(res, bias, E, K)
    lg = _logits(res["scores"], bias)
    for r in range(x.shape[0]):
        sel = res["sel"][r].tolist()
        if case == "nan_on_10":
            assert not set(sel) & set(nan.tolist())
        else:
            nk = len(keep)
            assert sel[:nk] == keep[np.argsort(-lg[r, keep], kind="stable")].tolist(), sel          # the finite ones, in logit order
            assert sel[nk:] == masked[:K - nk].tolist(), sel                                        # then the lowest masked indices
    if case == "nan_on_10":
        _check_weights(res, bias)


# ------------------------------------------------------------------------------------------------
# moe_build_slots / moe_scatter
# ------------------------------------------------------------------------------------------------

def _slots_case(name):
    rng = np.random.default_rng(len(name))
    if name == "E128":
        # zeros, ones, one expert at exactly max_rows, one at max_rows + 1 (refused), 35 and 40 rows span three slots, 17 two, 16 exactly one
        E, m, max_rows, bsz = 128, 16, 40, 48
        counts = np.zeros(E, dtype=np.int64)
        counts[[3, 64, 127, 70, 9]] = [40, 41, 35, 17, 16]
        counts[[0, 100]] = [20, 3]
        counts[rng.permutation(np.setdiff1d(np.arange(E), [0, 3, 9, 64, 70, 100, 127]))[:20]] = 1
        assert counts.sum() == 192
    elif name == "E512":
        # more than 256 slots (the j += 256 loops) and more than 256 experts (the e += 256 loops); two experts above max_rows
        E, m, max_rows, bsz = 512, 4, 64, 512
        p = rng.random(E) * (rng.random(E) > 0.2)
        counts = rng.multinomial(4096 - 65 - 130 - 64, p / p.sum()).astype(np.int64)
        counts[300] += 65; counts[7] += 130; counts[511] += 64
        counts[[0, 255, 256]] = [0, counts[0] + counts[255] + counts[256], 0]
        assert counts.sum() == 4096 and counts.max() > 64 and (counts > 0).sum() > 256
    elif name == "E1":
        E, m, max_rows, bsz, counts = 1, 4, 8, 3, np.array([7], dtype=np.int64)
    elif name == "E1_refused":
        E, m, max_rows, bsz, counts = 1, 4, 6, 3, np.array([7], dtype=np.int64)
    else:
        E, m, max_rows, bsz, counts = 8, 1, 1, 1, np.array([0, 0, 0, 0, 0, 1, 0, 0], dtype=np.int64)        # T == 1
    T = int(counts.sum())
    return E, m, max_rows, counts, rng.integers(0, bsz, T).astype(np.int64)


@pytest.mark.parametrize("name", ["E128", "E512", "E1", "E1_refused", "T1"])
def test_moe_build_slots_equals_the_restatement(dev, name):
    from exllamav3_amd import ext
    E, m, max_rows, counts, toks = _slots_case(name)
    T = toks.shape[0]
    se, st, rm = ext.moe_build_slots(_T(counts, dev), _T(toks, dev), max_rows, m)
    torch.cuda.synchronize()
    ns = R.ns_max(E, T, m)
    assert se.shape == (ns,) and st.shape == (ns * m,) and rm.shape == (T,)
    assert se.dtype == torch.long and st.dtype == torch.long and rm.dtype == torch.int32
    se_ref, st_ref, rm_ref = R.build_slots(counts, toks, max_rows, m, ns)
    if name == "E512":
        assert (se_ref >= 0).sum() > 256
    assert np.array_equal(_np(se), se_ref)
    assert np.array_equal(_np(st), st_ref)
    assert np.array_equal(_np(rm), rm_ref)


@pytest.mark.parametrize("hidden", [256, 2880])
def test_moe_scatter_short_and_long_assignment_lists(dev, hidden):
    """One launch whose tokens have 0, 1, 8, 64, 65 and 200 mapped assignments (the 64-entry list on both sides of its limit, and the walk over all
    assignments behind it), every token with some unmapped (-1) assignments as well, against the float64 sum in ascending p.  hidden 2880: 720 float4
    columns, the last pass of the 1024-column stride is partial.  Bound per element: (n + 2) * 2^-24 * (|out0| + sum |w d|) -- n fp32 products and n fp32
    additions, each rounding at most 2^-24 of a partial sum that the absolute sum bounds."""
    from exllamav3_amd import ext
    rng = np.random.default_rng(hidden)
    valid = [0, 1, 8, 64, 65, 200]
    extra = [3, 2, 5, 7, 4, 6]                                               # unmapped assignments per token
    tok = np.concatenate([np.full(v + x, t) for t, (v, x) in enumerate(zip(valid, extra))]).astype(np.int64)
    mapped = np.concatenate([np.r_[np.ones(v, bool), np.zeros(x, bool)] for v, x in zip(valid, extra)])
    order = rng.permutation(tok.shape[0])
    tok, mapped = tok[order], mapped[order]
    T, rows = tok.shape[0], 400
    rm = np.where(mapped, rng.integers(0, rows, T), -1).astype(np.int32)
    assert rm.max() < rows
    D = rng.standard_normal((rows, hidden)).astype(np.float32)
    w = rng.uniform(-1.0, 1.0, T).astype(np.float16)
    out0 = rng.standard_normal((len(valid), hidden)).astype(np.float32)
    ref = R.scatter(D, rm, tok, w, out0)
    mag, n = R.scatter_abs(D, rm, tok, w, out0)
    assert n.tolist() == valid
    outs = []
    for _ in range(2):                                                       # fresh copies: the second call reproduces the first bit for bit
        out = _T(out0, dev)
        ext.moe_scatter(_T(D, dev), _T(rm, dev), _T(tok, dev), _T(w, dev), out)
        torch.cuda.synchronize()
        outs.append(_np(out))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0][0], out0[0])                               # the token without mapped assignments
    tol = (n[:, None] + 2) * 2.0 ** -24 * mag
    err = np.abs(outs[0].astype(np.float64) - ref)
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())


# ------------------------------------------------------------------------------------------------
# dispatch end to end: 128 experts, top-8
# ------------------------------------------------------------------------------------------------

H, I, E128, TOP, BITS = 256, 384, 128, 8, 4


class _Block:
    """One 128-expert block for the whole file, and the oracle's view of it (each expert's reconstructed matrices are decoded once)."""

    def __init__(self, dev):
        from exllamav3_amd.moe_path import SyntheticEXL3MoE
        self.moe = SyntheticEXL3MoE(H, I, experts=E128, top_k=TOP, K=BITS, cb=2, device=dev, seed=128)
        self.router = _np(self.moe.router)
        self._w = {}

    def _lin(self, kind, e, x, out_fp32=False):
        L = getattr(self.moe, kind)[e]
        if (kind, e) not in self._w:
            self._w[kind, e] = (_np(L.trellis), _np(L.suh), _np(L.svh), o.reconstruct(_np(L.trellis), L.K, 2))
        tr, suh, svh, w_hat = self._w[kind, e]
        return o.linear_forward(x, tr, suh, svh, L.K, 2, out_fp32=out_fp32, w_hat=w_hat)

    def expert(self, e, x):
        """down_e(silu(gate_e(x)) * up_e(x)), fp32 (rows, H)."""
        g = self._lin("gate", e, x).astype(np.float32); u = self._lin("up", e, x).astype(np.float32)
        return self._lin("down", e, (g / (1 + np.exp(-g)) * u).astype(np.float16), out_fp32=True)

    def routed(self, x, sel, w):
        """The oracle's per-assignment composition on a given routing: sum_j w[t, j] * expert(sel[t, j], x[t])."""
        ref = np.zeros((x.shape[0], H), dtype=np.float32)
        for t in range(x.shape[0]):
            for j in range(sel.shape[1]):
                ref[t] += np.float32(w[t, j]) * self.expert(int(sel[t, j]), x[t:t + 1])[0]
        return ref

    def check_routing(self, x_in):
        """The block's own router launch (moe.scores / sel / w / sel2) on x_in."""
        res = dict(scores=_np(self.moe.scores), sel=_np(self.moe.sel), w=_np(self.moe.w), gu=_np(self.moe.sel2))
        _check_scores(res, x_in, self.router)
        _check_selection(res, None, E128, TOP)
        _check_weights(res, None)
        return res


@pytest.fixture(scope="module")
def block(dev):
    return _Block(dev)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.sqrt((ref.astype(np.float64) ** 2).mean()))


@pytest.mark.parametrize("tokens", [1, 3])
def test_moe_block_forward_128_experts_top8(dev, block, tokens):
    """SyntheticEXL3MoE.forward at 128 experts x top-8 (8 / 24 slots, pointer tables of 128 and 256 entries): the returning form (indexed gate|up
    exl3_mgemm, weighted exl3_mgemm_act with the slot reduction) and the add_into form (exl3_mgemm_act_deferred + glue_resid_moe with top_k = 8), each
    against the oracle's composition on the launch's own selection."""
    moe = block.moe
    x = torch.randn((tokens, H), device=dev, generator=torch.Generator(device=dev).manual_seed(100 + tokens)).half()
    xs = _np(x)
    y = _np(moe.forward(x).float()).copy()
    res = block.check_routing(xs)
    ref = block.routed(xs, res["sel"], res["w"])
    assert _rel(y, ref) < 2e-2
    # add_into: the residual stream receives the block's output, ss_part the block sums of squares of the new residual
    rms = float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
    r0 = (np.random.default_rng(tokens).standard_normal((tokens, H)) * rms).astype(np.float16)
    resid = _T(r0, dev); ss = torch.full((tokens, H // 128), float("nan"), dtype=torch.float, device=dev)
    assert moe.forward(x, add_into=(resid, ss)) is None
    res2 = block.check_routing(xs)
    assert _same_bits(res, res2)
    r1 = _np(resid).astype(np.float32)
    # (the residual is rounded to fp16 once more: half an ulp of |r0 + y| <= 2^-11 * max|r1|, next to the 2e-2 rms bar)
    assert np.abs(r1 - r0.astype(np.float32) - ref).max() < 2e-2 * rms + 2.0 ** -11 * np.abs(r1).max()
    assert np.allclose(_np(ss), (r1.astype(np.float64) ** 2).reshape(tokens, H // 128, 128).sum(-1), rtol=SS_RTOL, atol=0)


def test_moe_block_forward_fx_128_experts_top8(dev, block):
    """forward_fx (router on the fixed-point residual, deferred indexed gate|up over 16 slots, weighted down launch adding into the accumulator with
    integer atomics) for one token: the accumulator's increment against the oracle on the launch's own normalised row and selection."""
    moe = block.moe
    rng = np.random.default_rng(7)
    xh = (rng.standard_normal((1, H)) * 2).astype(np.float16)
    norm_w = (1 + 0.1 * rng.standard_normal(H)).astype(np.float16)
    R0 = np.rint(xh.astype(np.float64) * 2.0 ** 32).astype(np.int64)
    Rd = _T(R0, dev)
    ss = torch.full((1, H // 128), float("nan"), dtype=torch.float, device=dev); xn = torch.empty((1, H), dtype=torch.half, device=dev)
    moe.forward_fx(Rd, _T(norm_w, dev), EPS, ss, xn)
    torch.cuda.synchronize()
    xn_np = _np(xn)
    xn_ref = o.rms_norm(xh, norm_w, EPS).astype(np.float32)
    assert np.abs(xn_np.astype(np.float32) - xn_ref).max() <= 2e-3 * np.abs(xn_ref).max()
    assert np.allclose(_np(ss), (xh.astype(np.float64) ** 2).reshape(1, H // 128, 128).sum(-1), rtol=SS_RTOL, atol=0)
    res = block.check_routing(xn_np)
    ref = block.routed(xn_np, res["sel"], res["w"])
    got = ((_np(Rd) - R0).astype(np.float64) / 2.0 ** 32).astype(np.float32)
    assert _rel(got, ref) < 2e-2


def test_exl3_moe_op_128_experts_routed_on_the_device(dev, block):
    """ext.exl3_moe for 24 tokens routed on the device (routing_std at 128 x top-8), the assignments sorted by expert as the reference's caller sorts
    them; max_tokens_per_expert is one below the busiest expert's count, so at least one expert is refused while its tokens' other assignments
    still land; two further rows of the batch are not routed at all and must stay untouched."""
    from exllamav3_amd import ext
    moe = block.moe
    bsz, routed = 26, 24
    rng = np.random.default_rng(24)
    x = rng.standard_normal((bsz, H)).astype(np.float16)
    dx = _T(x, dev)
    sc = torch.empty((routed, E128), dtype=torch.half, device=dev); sel = torch.empty((routed, TOP), dtype=torch.long, device=dev)
    wt = torch.empty((routed, TOP), dtype=torch.half, device=dev)
    ext.routing_std(dx[:routed], moe.router, sc, sel, wt)
    flat = sel.reshape(-1)
    order = torch.argsort(flat, stable=True)
    token_sorted = torch.div(order, TOP, rounding_mode="floor").contiguous()
    weight_sorted = wt.reshape(-1)[order].contiguous()
    counts = torch.bincount(flat, minlength=E128)
    cn = _np(counts)
    max_rows = int(cn.max()) - 1
    assert max_rows >= 1 and (cn > max_rows).sum() >= 1 and cn.sum() == routed * TOP
    out0 = rng.standard_normal((bsz, H)).astype(np.float32)
    out = _T(out0, dev)
    tmp_s = torch.empty((4, max_rows, H), dtype=torch.half, device=dev); tmp_i = torch.empty((4, max_rows, I), dtype=torch.half, device=dev)
    ext.exl3_moe(dx, out, torch.cat([counts, counts.new_zeros(1)]), token_sorted, weight_sorted, tmp_s, tmp_s, tmp_i, tmp_i, ext.MOE_ACT_SILU,
                 BITS, BITS, BITS, moe.g_B, moe.g_suh, moe.g_svh, moe.u_B, moe.u_suh, moe.u_svh, moe.d_B, moe.d_suh, moe.d_svh,
                 False, True, False, True, False, True, 0.0, 3)
    torch.cuda.synchronize()
    got = _np(out)
    sel_np, w_np = _np(sel), _np(wt)
    _check_selection(dict(scores=_np(sc), sel=sel_np, gu=None), None, E128, TOP)
    refused = np.flatnonzero(cn > max_rows)
    ref = out0.copy()
    for t in range(routed):
        for j in range(TOP):
            e = int(sel_np[t, j])
            if e not in refused:
                ref[t] += np.float32(w_np[t, j]) * block.expert(e, x[t:t + 1])[0]
    delta = ref - out0
    assert _rel(got[:routed] - out0[:routed], delta[:routed]) < 2e-2
    hit = np.flatnonzero(np.isin(sel_np, refused).any(1))                    # tokens that lost an assignment to a refused expert: the others landed
    assert hit.size >= 2 and (np.abs(got[hit] - out0[hit]).max(1) > 0).all()
    assert np.array_equal(got[routed:], out0[routed:])


def test_bc_blocksparse_mlp_run_bszN_128_experts_top8(dev, block):
    """BC_BlockSparseMLP.run_bszN at 128 experts x top-8: 1 and 3 tokens with every expert local, then as the rank that holds experts [32, 96) with a
    selection that has members below, inside and above the range (the partial sum over the local ones)."""
    from exllamav3_amd import ext
    moe = block.moe
    rng = np.random.default_rng(96)
    MAXB = ext.BC_BlockSparseMLP.MAX_BSZN
    bszn = MAXB * TOP
    th = torch.empty((bszn, H), dtype=torch.half, device=dev); ti = torch.empty((2 * bszn, I), dtype=torch.half, device=dev)
    ta = torch.empty((bszn, I), dtype=torch.half, device=dev); to_ = torch.empty((bszn, H), dtype=torch.float, device=dev)
    bcl = lambda l: ext.BC_LinearEXL3(l.trellis, l.suh, l.svh, BITS, None, l.mcg, l.mul1, None)
    gates, ups, downs = [bcl(l) for l in moe.gate], [bcl(l) for l in moe.up], [bcl(l) for l in moe.down]

    def make(min_e, max_e):
        lo, hi = (0, E128) if min_e < 0 else (min_e, max_e)                   # a rank's pointer tables hold its local experts only
        loc = lambda t: t[lo:hi].contiguous()
        return ext.BC_BlockSparseMLP(
            th, th[:bszn].view(bszn, 1, H), ti, ti[:bszn].view(bszn, 1, I), ti[bszn:2 * bszn].view(bszn, 1, I), ta[:bszn].view(bszn, 1, I), ta,
            to_[:bszn].view(bszn, 1, H), to_, None, None, torch.empty((H, I), dtype=torch.half, device=dev), torch.empty((I, H), dtype=torch.half, device=dev),
            min_e, max_e, loc(moe.g_B), loc(moe.g_suh), loc(moe.g_svh), BITS, False, True, loc(moe.u_B), loc(moe.u_suh), loc(moe.u_svh), BITS, False, True,
            loc(moe.d_B), loc(moe.d_suh), loc(moe.d_svh), BITS, False, True, True, False, False, None, None, 0.0, gates[lo:hi], ups[lo:hi], downs[lo:hi],
            None, None, None, torch.empty((bszn, H), dtype=torch.half, device=dev))

    bc = make(-1, -1)
    for bsz in (1, 3):
        x = rng.standard_normal((bsz, H)).astype(np.float16)
        sel = np.stack([rng.permutation(E128)[:TOP] for _ in range(bsz)]).astype(np.int64)
        wts = rng.uniform(0.05, 0.3, (bsz, TOP)).astype(np.float16)
        bc.run_bszN(_T(x, dev), _T(sel, dev), _T(wts, dev))
        got = _np(to_[:bsz]).copy()
        assert _rel(got, block.routed(x, sel, wts)) < 2e-2, bsz
    bc_ep = make(32, 96)
    x = rng.standard_normal((1, H)).astype(np.float16)
    sel = np.array([[3, 40, 95, 100, 32, 127, 64, 31]], np.int64)
    wts = rng.uniform(0.05, 0.3, (1, TOP)).astype(np.float16)
    bc_ep.run_bszN(_T(x, dev), _T(sel, dev), _T(wts, dev))
    local = [j for j in range(TOP) if 32 <= sel[0, j] < 96]
    assert [int(sel[0, j]) for j in local] == [40, 95, 32, 64]
    ref = block.routed(x, sel[:, local], wts[:, local])
    assert _rel(_np(to_[:1]).copy(), ref) < 2e-2
