"""Logit processors without a GPU: the library's new entries and their argument errors, the numpy restatement of exl3_logit_process (tests/_logit_proc_ref.py)
against a literal float32 transcription of the reference's two penalty kernels (rep_pen.cu: sequential loop, 1e-30 guards and all -- test code of this project),
the window edges, the collapse rules of sampling.LogitProcessors, and the names exllamav3_amd.ext gains."""
import numpy as np
import pytest
import _logit_proc_ref as LP

F = np.float32
NEG = F(-np.inf)


# ---- the reference's kernels, transcribed literally in float32 (one thread after another) -----------------------------------------------------------------
def _ref_factor(n, i, S, D):
    if D > 0:
        factor = F(1.0) - (F(n - i) - F(S)) / F(D)
    else:
        factor = F(1.0)
    return min(max(factor, F(0.0)), F(1.0))


def ref_apply_rep_pens(logits, past, rep_p, S, D):
    vocab, n = logits.shape[0], len(past)
    factors = np.zeros((vocab,), dtype=F)
    for i in range(n):
        if i <= n - S - D:
            continue
        t = int(past[i])
        if t < 0 or t >= vocab:
            continue
        if n - i <= S:
            factors[t] = F(1.0)
        else:
            factors[t] = max(factors[t], _ref_factor(n, i, S, D))
    rep_p = F(rep_p)
    v = logits.astype(F)
    with np.errstate(all="ignore"):
        w = np.where(v > F(0), v / rep_p, v * rep_p).astype(F)
        f = (factors.astype(np.float64) + 1e-30).astype(F)                       # (float + double literal, rounded back to float)
        f1 = ((F(1.0) - f).astype(F).astype(np.float64) + 1e-30).astype(F)
        return ((v * f1).astype(F) + (w * f).astype(F)).astype(F)


def ref_apply_pres_freq_pens(logits, past, pres_p, freq_p, S, D):
    vocab, n = logits.shape[0], len(past)
    frequency = np.zeros((vocab,), dtype=F)
    presence = np.zeros((vocab,), dtype=F)
    pres_p, freq_p = F(pres_p), F(freq_p)
    for i in range(n):
        if i <= n - S - D:
            continue
        t = int(past[i])
        if t < 0 or t >= vocab:
            continue
        factor = _ref_factor(n, i, S, D)
        frequency[t] = F(frequency[t] + F(factor * freq_p))
        presence[t] = max(presence[t], F(factor * pres_p))
    with np.errstate(all="ignore"):
        v = logits.astype(F)
        v = (v - frequency).astype(F)
        return (v - presence).astype(F)


def _counts(past, size, S, D):
    past = np.asarray(past, dtype=np.int64).reshape(-1)
    n = past.shape[0]
    c = np.zeros((size,), dtype=np.int64)
    if n:
        dist = n - np.arange(n)
        ok = (dist < S + D) & (past >= 0) & (past < size)
        np.add.at(c, past[ok], 1)
    return c


def _case(rng, k):
    V = 4096
    logits = (rng.standard_normal(V) * 2.0).astype(np.float16)
    if k % 3 == 0:
        logits[rng.integers(0, V, 40)] = -np.inf
    n = int(rng.integers(0, 601)) if k % 7 else 0
    pool = rng.integers(0, V, 48)
    past = np.where(rng.random(n) < 0.7, pool[rng.integers(0, 48, n)], rng.integers(-5, V + 50, n))
    S = [0, 1, 5, 100, 10 ** 8][int(rng.integers(0, 5))]
    D = [0, 1, 7, 200][int(rng.integers(0, 4))]
    return V, logits, past, S, D


def test_restatement_against_the_transcribed_reference_kernels():
    rng = np.random.default_rng(20261016)
    worst_rep = worst_pf = 0.0
    for k in range(60):
        V, logits, past, S, D = _case(rng, k)
        src = logits if k % 2 else logits.astype(F)
        # repetition penalty
        rep_p = float(rng.uniform(1.05, 2.0))
        got = LP.process_row(src, V, past, rep=(rep_p, S, D), out_dtype=F)
        if S + D > 0:
            exp = ref_apply_rep_pens(src, past, rep_p, S, D)
            assert np.array_equal(np.isfinite(got), np.isfinite(exp)) and np.array_equal(got[~np.isfinite(got)], exp[~np.isfinite(exp)]), k
            fin = np.isfinite(exp)
            err = np.abs(got[fin].astype(np.float64) - exp[fin].astype(np.float64))
            bound = 2.0 ** -22 * np.abs(exp[fin].astype(np.float64))
            assert (err <= bound).all(), (k, S, D, float((err - bound).max()))
            nz = np.abs(exp[fin]) > 0
            if nz.any():
                worst_rep = max(worst_rep, float((err[nz] / np.abs(exp[fin][nz].astype(np.float64))).max()))
        else:
            assert LP.same_bits(got, src.astype(F))                                  # the reference's SS_NoOp rule (custom.py:790-793)
        # presence / frequency
        pres_p, freq_p = float(rng.uniform(0.0, 1.5)), float(rng.uniform(0.0, 0.6))
        got = LP.process_row(src, V, past, pf=(pres_p, freq_p, S, D), out_dtype=F)
        if S + D > 0:
            exp = ref_apply_pres_freq_pens(src, past, pres_p, freq_p, S, D)
            assert np.array_equal(np.isfinite(got), np.isfinite(exp)) and np.array_equal(got[~np.isfinite(got)], exp[~np.isfinite(exp)]), k
            fin = np.isfinite(exp)
            c = _counts(past, V, S, D).astype(np.float64)
            v0 = np.abs(src.astype(np.float64))
            bound = (c + 3) * 2.0 ** -24 * np.maximum(v0, c * abs(freq_p) + abs(pres_p))
            err = np.zeros_like(bound)
            err[fin] = np.abs(got[fin].astype(np.float64) - exp[fin].astype(np.float64))
            assert (err[fin] <= bound[fin]).all(), (k, S, D, float((err[fin] - bound[fin]).max()))
            worst_pf = max(worst_pf, float(err[fin].max()))
        else:
            assert LP.same_bits(got, src.astype(F))
    print("restatement vs transcribed reference: worst relative (rep)", worst_rep, "worst absolute (pres / freq)", worst_pf)


@pytest.mark.parametrize("S,D", [(5, 0), (5, 7), (1, 1), (0, 3), (3, 200)])
def test_window_edges(S, D):
    """dist = S - 1, S, S + 1, S + D - 1, S + D: which count, and with which integer weight; the transcribed reference agrees on what counts."""
    V = 64
    Dn = max(D, 1)
    for dist in sorted({S - 1, S, S + 1, S + D - 1, S + D, S + D + 1}):
        if dist < 1:
            continue
        n = dist + 3
        past = np.full((n,), -1, dtype=np.int64)
        past[n - dist] = 9                                                          # one in-range token at distance dist
        pmax, fsum, dn = LP.window_tables(past, V, S, D)
        counts = dist < S + D                                                       # (D = 0: dist <= S - 1 -- the reference's quirk, kept)
        num = (Dn if dist <= S else D - (dist - S)) if counts else 0
        assert dn == Dn and int(pmax[9]) == num and int(fsum[9]) == num and int(pmax.sum()) == num, (S, D, dist)
        logits = np.full((V,), 2.0, dtype=F)
        ref = ref_apply_rep_pens(logits, past, 1.5, S, D)
        assert (ref[9] != F(2.0)) == counts, (S, D, dist)
        got = LP.process_row(logits, V, past, rep=(1.5, S, D), out_dtype=F)
        assert (got[9] != F(2.0)) == counts and abs(float(got[9]) - float(ref[9])) <= 2.0 ** -22 * abs(float(ref[9]))
    # two occurrences: the maximum for presence / repetition, the sum for frequency
    past = np.array([9, 3, 9, 3, 3], dtype=np.int64)
    pmax, fsum, _ = LP.window_tables(past, V, 2, 3)                                  # dist 5 4 3 2 1 -> counts iff dist < 5: nums -, 1, 2, 3, 3
    assert int(pmax[9]) == 2 and int(fsum[9]) == 2 and int(pmax[3]) == 3 and int(fsum[3]) == 1 + 3 + 3


def test_identity_when_everything_is_off():
    from exllamav3_amd.sampling import LogitProcessors
    rng = np.random.default_rng(1)
    row = (rng.standard_normal(1000) * 2).astype(np.float16)
    row[:6] = np.array([0.0, -0.0, 6e-8, -6e-8, -np.inf, np.nan], dtype=np.float16)
    for p in (LogitProcessors(), LogitProcessors(rep_p=1.0, rep_sustain=50), LogitProcessors(rep_p=1.3, rep_sustain=0, rep_decay=0),
              LogitProcessors(pres_p=0.5, freq_p=0.5, pf_sustain=0), LogitProcessors(logit_bias={3: 0.0, 4: float("nan"), 5: 1e39, -7: 2.0})):
        assert not p.rep_on and not p.pf_on
        out = LP.process_row(row, 1000, [1, 2, 3, 3], rep=(p.rep_p, p.rep_sustain, p.rep_decay), pf=(p.pres_p, p.freq_p, p.pf_sustain, p.pf_decay))
        assert LP.same_bits(out, row) and np.array_equal(out.view(np.uint16)[:5], row.view(np.uint16)[:5])
    assert LogitProcessors().is_noop and LogitProcessors(logit_bias={3: 0.0, 4: float("nan"), 5: 1e39}).is_noop


def test_logit_processors_collapse_and_validate():
    from exllamav3_amd.sampling import LogitProcessors
    p = LogitProcessors(rep_p=1.3, rep_sustain=16, rep_decay=8, freq_p=0.3)
    assert p.rep_on and p.pf_on and p.needs_history and not p.is_noop
    assert (p.rep_p, p.rep_sustain, p.rep_decay) == (1.3, 16, 8) and (p.pres_p, p.freq_p, p.pf_sustain, p.pf_decay) == (0.0, 0.3, 10 ** 8, 0)
    # the reference's no-op rules (custom.py:790-793, :855-858)
    assert not LogitProcessors(rep_p=1.0, rep_sustain=16).rep_on and not LogitProcessors(rep_p=1.3, rep_sustain=0, rep_decay=0).rep_on
    assert LogitProcessors(rep_p=1.3, rep_sustain=0, rep_decay=4).rep_on
    assert not LogitProcessors(pres_p=0.0, freq_p=0.0).pf_on and not LogitProcessors(pres_p=1.0, pf_sustain=0, pf_decay=0).pf_on
    assert LogitProcessors(pres_p=0.2).pf_on
    # bias: 0, NaN and what overflows fp32 to +inf are dropped (custom.py:586-595); -inf and large negatives stay; bans are -inf and win
    b = LogitProcessors(logit_bias={1: 0.0, 2: float("nan"), 3: 1e39, 4: float("inf"), 5: -1e39, 6: float("-inf"), 7: 2.5, 8: 1.0, 200: 1.0, -1: 1.0},
                        ban_token_ids=[8, 9, 10 ** 6])
    assert b.bias == {5: -1e39, 6: float("-inf"), 7: 2.5, 8: float("-inf"), 200: 1.0, -1: 1.0, 9: float("-inf"), 10 ** 6: float("-inf")}
    assert not b.needs_history and not b.is_noop
    vec, bm = b.tensors(100, "cpu")                                                  # ids outside the vocabulary are ignored
    assert bm is None and vec.dtype.is_floating_point and vec.shape == (100,)
    exp = np.zeros((100,), dtype=F)
    exp[[5, 6, 8, 9]] = -np.inf
    exp[7] = 2.5
    assert np.array_equal(vec.numpy(), exp)
    assert b.tensors(100, "cpu")[0] is vec                                           # built once per (vocabulary, device)
    for bad in (dict(rep_p=0.0), dict(rep_p=float("nan")), dict(rep_p=-1.0), dict(pres_p=float("inf")), dict(freq_p=float("nan")), dict(rep_sustain=-1),
                dict(pf_decay=-3), dict(rep_sustain=2 ** 31), dict(rep_sustain=2 ** 30, rep_decay=2 ** 30), dict(pf_sustain=1.5)):
        with pytest.raises(ValueError):
            LogitProcessors(**bad)
    import torch
    with pytest.raises(ValueError):
        LogitProcessors(bitmask=torch.zeros((1, 4), dtype=torch.int64))
    with pytest.raises(ValueError):
        LogitProcessors(bitmask=torch.zeros((4,), dtype=torch.int32))
    assert not LogitProcessors(bitmask=torch.zeros((1, 4), dtype=torch.int32)).is_noop


def test_new_entries_are_exported_and_report_argument_errors_without_gpu():
    from exllamav3_amd import _lib
    l = _lib.lib()
    assert "exl3_logit_process" in _lib.declared_symbols() and "exl3_gen_feed_stop" in _lib.declared_symbols()
    assert hasattr(l, "exl3_logit_process") and hasattr(l, "exl3_gen_feed_stop")
    A = 4096                                                                         # (an aligned non-null address: never dereferenced, the checks come first)

    def P(**kw):
        a = dict(lin=A, in32=0, lout=A, out32=0, m=1, ld=128, size=128, pa=None, lda=0, len_a=0, pb=None, ldb=0, len_b=0, dev=None, bias_=0, rep_p=1.0, rs=0, rd=0,
                 pres=0.0, freq=0.0, ps=0, pd=0, bias=None, bm=None, bm_rows=0, bm_words=0)
        a.update(kw)
        return l.exl3_logit_process(a["lin"], a["in32"], a["lout"], a["out32"], a["m"], a["ld"], a["size"], a["pa"], a["lda"], a["len_a"], a["pb"], a["ldb"], a["len_b"],
                                    a["dev"], a["bias_"], a["rep_p"], a["rs"], a["rd"], a["pres"], a["freq"], a["ps"], a["pd"], a["bias"], a["bm"], a["bm_rows"],
                                    a["bm_words"], None)

    assert P(m=17) == -1 and b"m must be in [1, 16]" in l.exl3_last_error()
    assert P(m=0) == -1
    assert P(size=129) == -1 and b"size <= ld" in l.exl3_last_error()
    assert P(ld=100, size=100) == -1 and b"multiple of 8" in l.exl3_last_error()
    assert P(lin=A + 2) == -1 and b"16-byte aligned" in l.exl3_last_error()
    assert P(lout=A + 8) == -1 and b"16-byte aligned" in l.exl3_last_error()
    assert P(lin=None) == -1 and b"null pointer" in l.exl3_last_error()
    assert P(out32=1) == -1 and b"in place" in l.exl3_last_error()
    assert P(pa=None, len_a=3, lda=3) == -1 and b"past_a" in l.exl3_last_error()
    assert P(pb=A, ldb=4, len_b=5) == -1 and b"past_b" in l.exl3_last_error()
    assert P(dev=A) == -1 and b"without past_b" in l.exl3_last_error()
    assert P(rep_p=0.0) == -1 and b"rep_p must be positive" in l.exl3_last_error()
    assert P(rep_p=1.3, rs=-1) == -1 and b"must not be negative" in l.exl3_last_error()
    assert P(rep_p=1.3, rs=2 ** 30, rd=2 ** 30) == -1 and b"fit an int32" in l.exl3_last_error()
    # a window whose integer frequency sum could pass 2^32: min(S + D, len_a + ldb) * max(D, 1)
    assert P(pb=A, ldb=2 ** 29, freq=0.5, ps=2 ** 29, pd=2 ** 20) == -1 and b"integer frequency sum" in l.exl3_last_error()
    assert P(bm=A, bm_rows=2, bm_words=4) == -1 and b"bitmask" in l.exl3_last_error()
    assert P(bm=A, bm_rows=1, bm_words=0) == -1
    with pytest.raises(RuntimeError):
        _lib.check(P(m=17))

    def G(n_stop, stop=A, done=A, live=A, m=1):
        #                           sampled forced flen m embed vocab hidden x0 out olen pos seq att inv step stop n_stop done pad live stream
        return l.exl3_gen_feed_stop(A, None, 0, m, A, 10, 64, A, None, 0, None, None, None, A, A, stop, n_stop, done, 0, live, None)

    assert G(65) == -1 and b"at most 64 stop ids" in l.exl3_last_error()
    assert G(-1) == -1
    assert G(2, stop=None) == -1
    assert G(1, done=None) == -1 and b"null pointer" in l.exl3_last_error()
    assert G(1, live=None) == -1
    assert G(1, m=17) == -1 and b"m must be in [1, 16]" in l.exl3_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(G(65))


def test_deterministic_reference_names_resolve_and_noise_drawing_names_do_not():
    from exllamav3_amd import ext
    for name in ("apply_rep_pens", "apply_pres_freq_pens", "apply_logit_bitmask"):
        assert callable(getattr(ext, name)), name
    for name in ("argmax_sample", "gumbel_sample", "fused_sampler", "gumbel_noise_f16", "gumbel_noise_f32", "gumbel_noise_log"):
        assert name not in vars(ext), name
        with pytest.raises(AttributeError):
            getattr(ext, name)
    import torch
    lg = torch.zeros((2, 128))
    with pytest.raises(RuntimeError):                                                # the reference's checks come before any device work
        ext.apply_rep_pens(lg, lg, torch.zeros((1, 4), dtype=torch.long), 1.2, 10, 0)
