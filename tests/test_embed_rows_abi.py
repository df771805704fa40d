"""exl3_embed_rows (csrc/exl3_sampler.hip; sampling.embed_rows) at the C ABI: exported, declared, and its argument errors reported before any device work."""
import pytest


def test_embed_rows_is_exported_and_declared():
    from exllamav3_amd import _lib
    l = _lib.lib()
    assert "exl3_embed_rows" in _lib.declared_symbols()
    assert hasattr(l, "exl3_embed_rows")
    from exllamav3_amd import sampling
    assert callable(sampling.embed_rows)


def test_embed_rows_reports_argument_errors_without_gpu():
    from exllamav3_amd import _lib
    l = _lib.lib()
    A = 4096                                                                         # (an aligned non-null address: never dereferenced, the checks come first)

    def E(**kw):
        a = dict(ids=A, ld=32, col0=0, T=8, m=1, embed=A, vocab=100, hidden=64, out=A, invalid=A)
        a.update(kw)
        return l.exl3_embed_rows(a["ids"], a["ld"], a["col0"], a["T"], a["m"], a["embed"], a["vocab"], a["hidden"], a["out"], a["invalid"], None)

    for nm in ("ids", "embed", "out", "invalid"):
        assert E(**{nm: None}) == -1 and b"null pointer" in l.exl3_last_error(), nm
    assert E(hidden=68) == -1 and b"multiple of 8" in l.exl3_last_error()
    assert E(hidden=0) == -1
    assert E(m=0) == -1 and b"m must be in [1, 16]" in l.exl3_last_error()
    assert E(m=17) == -1 and b"m must be in [1, 16]" in l.exl3_last_error()
    assert E(T=0) == -1 and b"T must be at least 1" in l.exl3_last_error()
    assert E(T=-3) == -1
    assert E(col0=-1) == -1 and b"inside the id matrix" in l.exl3_last_error()
    assert E(col0=25, T=8) == -1 and b"inside the id matrix" in l.exl3_last_error()
    assert E(embed=A + 2) == -1 and b"16-byte aligned" in l.exl3_last_error()
    assert E(out=A + 8) == -1 and b"16-byte aligned" in l.exl3_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(E(m=17))
