"""exl3_spec_accept / exl3_spec_draft_ngram / exl3_spec_round (csrc/exl3_spec.hip; sampling.spec_accept / spec_draft / spec_round) at the C ABI: exported,
declared, and their argument errors reported before any device work."""
import pytest

A = 4096                                                                             # (an aligned non-null address: never dereferenced, the checks come first)


def test_spec_entries_are_exported_and_declared():
    from exllamav3_amd import _lib, sampling
    l = _lib.lib()
    for name in ("exl3_spec_accept", "exl3_spec_draft_ngram", "exl3_spec_round"):
        assert name in _lib.declared_symbols(), name
        assert hasattr(l, name), name
        assert getattr(l, name).argtypes, name
    assert l.exl3_abi_version() == 4                                                 # only new symbols: the ABI version stays
    assert callable(sampling.spec_accept) and callable(sampling.spec_draft) and callable(sampling.spec_round)
    s = sampling.SpeculativeSettings()
    assert (s.num_draft_tokens, s.ngram_match_min, s.ngram_match_max, s.script) == (3, 2, 8, None)
    for bad in (dict(num_draft_tokens=0), dict(num_draft_tokens=16), dict(ngram_match_min=0), dict(ngram_match_min=9), dict(ngram_match_max=17)):
        with pytest.raises(ValueError):
            sampling.SpeculativeSettings(**bad)


def _accept(l, **kw):
    a = dict(sampled=A, in_tokens=A, m=4, vocab=1024, state=A, round=A, hist=A, max_ctx=512, tokens_out=A, max_new=48, stop_ids=None, n_stop=0)
    a.update(kw)
    return l.exl3_spec_accept(a["sampled"], a["in_tokens"], a["m"], a["vocab"], a["state"], a["round"], a["hist"], a["max_ctx"], a["tokens_out"], a["max_new"],
                              a["stop_ids"], a["n_stop"], None)


def _draft(l, **kw):
    a = dict(hist=A, max_ctx=512, script=None, k=3, match_min=2, match_max=8, m=4, state=A, max_new=48, in_tokens=A, embed=A, vocab=1024, hidden=512, x0=A,
             positions=A, cache_seqlens=A, attn_lens=A)
    a.update(kw)
    return l.exl3_spec_draft_ngram(a["hist"], a["max_ctx"], a["script"], a["k"], a["match_min"], a["match_max"], a["m"], a["state"], a["max_new"], a["in_tokens"],
                                   a["embed"], a["vocab"], a["hidden"], a["x0"], a["positions"], a["cache_seqlens"], a["attn_lens"], None)


def _round(l, **kw):
    a = dict(sampled=A, in_tokens=A, m=4, vocab=1024, state=A, round=A, hist=A, max_ctx=512, tokens_out=A, max_new=48, stop_ids=None, n_stop=0, script=None, k=3,
             match_min=2, match_max=8, embed=A, hidden=512, x0=A, positions=A, cache_seqlens=A, attn_lens=A)
    a.update(kw)
    return l.exl3_spec_round(a["sampled"], a["in_tokens"], a["m"], a["vocab"], a["state"], a["round"], a["hist"], a["max_ctx"], a["tokens_out"], a["max_new"],
                             a["stop_ids"], a["n_stop"], a["script"], a["k"], a["match_min"], a["match_max"], a["embed"], a["hidden"], a["x0"], a["positions"],
                             a["cache_seqlens"], a["attn_lens"], None)


def test_spec_accept_reports_argument_errors_without_gpu():
    from exllamav3_amd import _lib
    l = _lib.lib()
    for nm in ("sampled", "in_tokens", "state", "round", "hist", "tokens_out"):
        assert _accept(l, **{nm: None}) == -1 and b"null pointer" in l.exl3_last_error(), nm
    for m in (0, 17, -1):
        assert _accept(l, m=m) == -1 and b"m must be in [1, 16]" in l.exl3_last_error()
    assert _accept(l, n_stop=65, stop_ids=A) == -1 and b"at most 64 stop ids" in l.exl3_last_error()
    assert _accept(l, n_stop=1, stop_ids=None) == -1 and b"at most 64 stop ids" in l.exl3_last_error()
    assert _accept(l, n_stop=-1) == -1
    assert _accept(l, vocab=0) == -1 and _accept(l, max_ctx=0) == -1 and _accept(l, max_new=-1) == -1
    with pytest.raises(RuntimeError):
        _lib.check(_accept(l, m=17))


@pytest.mark.parametrize("entry", ["draft", "round"])
def test_spec_draft_and_round_report_argument_errors_without_gpu(entry):
    from exllamav3_amd import _lib
    l = _lib.lib()
    E = {"draft": _draft, "round": _round}[entry]
    ptrs = ["hist", "state", "in_tokens", "embed", "x0", "positions", "cache_seqlens", "attn_lens"] + (["sampled", "round", "tokens_out"] if entry == "round" else [])
    for nm in ptrs:
        assert E(l, **{nm: None}) == -1 and b"null pointer" in l.exl3_last_error(), nm
    for m in (0, 17):
        assert E(l, m=m, k=0) == -1 and b"m must be in [1, 16]" in l.exl3_last_error()
    assert E(l, match_min=9, match_max=8) == -1 and b"match_min <= match_max" in l.exl3_last_error()
    assert E(l, match_min=0) == -1 and b"match_min <= match_max" in l.exl3_last_error()
    assert E(l, match_min=2, match_max=17) == -1 and b"match_max must be at most 16" in l.exl3_last_error()
    assert E(l, k=4, m=4) == -1 and b"k must be in [0, m - 1]" in l.exl3_last_error()
    assert E(l, k=16, m=16) == -1 and b"k must be in [0, m - 1]" in l.exl3_last_error()
    assert E(l, k=-1) == -1
    assert E(l, hidden=68) == -1 and b"multiple of 8" in l.exl3_last_error()
    assert E(l, embed=A + 2) == -1 and b"16-byte aligned" in l.exl3_last_error()
    assert E(l, x0=A + 8) == -1 and b"16-byte aligned" in l.exl3_last_error()
    if entry == "round":
        assert E(l, n_stop=65, stop_ids=A) == -1 and b"at most 64 stop ids" in l.exl3_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(E(l, match_max=17))
