"""CPU restatement (numpy) of the logit processors' contract (include/exl3_hip.h: exl3_logit_process): integer window tables, then float32 operations in the
stated order, every one rounded on its own, and one round-to-nearest-even conversion to the output type.  Not a port of the kernel: no spans, no atomics --
np.maximum.at / np.add.at over the whole vocabulary."""
import numpy as np

F = np.float32


def window_tables(past, size, S, D):
    """past: the row's ids, oldest first.  -> (pmax uint32 [size], fsum uint64 [size], Dn).  The token at index i of n has dist = n - i; it counts iff
    dist < S + D, with the weight numerator Dn = max(D, 1) if dist <= S else D - (dist - S)."""
    past = np.asarray(past, dtype=np.int64).reshape(-1)
    n = past.shape[0]
    Dn = max(int(D), 1)
    pmax = np.zeros((size,), dtype=np.uint32)
    fsum = np.zeros((size,), dtype=np.uint64)
    if n:
        dist = n - np.arange(n, dtype=np.int64)
        num = np.where(dist <= S, Dn, D - (dist - S))
        ok = (dist < S + D) & (past >= 0) & (past < size)
        assert (num[ok] >= 1).all() and (num[ok] <= Dn).all()
        np.maximum.at(pmax, past[ok], num[ok].astype(np.uint32))
        np.add.at(fsum, past[ok], num[ok].astype(np.uint64))
        assert int(fsum.max()) < 2 ** 32
    return pmax, fsum, Dn


def process_row(logits, size, past=(), rep=None, pf=None, bias=None, bitmask=None, out_dtype=np.float16):
    """logits: one row [ld] (float16 / float32).  rep = (rep_p, S, D), pf = (pres_p, freq_p, S, D), bias: float32 [size], bitmask: uint32 [words] (bit set =
    keep).  -> out_dtype [ld], columns [size, ld) = -inf."""
    logits = np.asarray(logits)
    ld = logits.shape[0]
    v = logits[:size].astype(F)
    with np.errstate(all="ignore"):
        if rep is not None and F(rep[0]) != F(1.0) and rep[1] + rep[2] > 0:
            rep_p = F(rep[0])
            pmax, _, Dn = window_tables(past, size, rep[1], rep[2])
            hit = (pmax > 0) & np.isfinite(v)
            w = np.where(v > F(0), v / rep_p, v * rep_p).astype(F)
            f = pmax.astype(F) / F(Dn)
            blend = (v * (F(1.0) - f)).astype(F) + (w * f).astype(F)
            v = np.where(hit, blend, v).astype(F)
        if pf is not None and (F(pf[0]) != F(0.0) or F(pf[1]) != F(0.0)) and pf[2] + pf[3] > 0:
            pres_p, freq_p = F(pf[0]), F(pf[1])
            pmax, fsum, Dn = window_tables(past, size, pf[2], pf[3])
            hit = (pmax > 0) & np.isfinite(v)
            fterm = (freq_p * (fsum.astype(F) / F(Dn)).astype(F)).astype(F)
            pterm = (pres_p * (pmax.astype(F) / F(Dn)).astype(F)).astype(F)
            pen = ((v - fterm).astype(F) - pterm).astype(F)
            v = np.where(hit, pen, v).astype(F)
        if bias is not None:
            v = (v + np.asarray(bias, dtype=F)[:size]).astype(F)
        if bitmask is not None:
            bm = np.asarray(bitmask).view(np.uint32).reshape(-1)
            t = np.arange(size)
            wi = t >> 5
            keep = np.zeros((size,), dtype=bool)
            inside = wi < bm.shape[0]
            keep[inside] = ((bm[wi[inside]] >> (t[inside] & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
            v = np.where(keep, v, F(-np.inf)).astype(F)
        out = np.full((ld,), -np.inf, dtype=out_dtype)
        out[:size] = v.astype(out_dtype)
    return out


def process(logits, size, pasts=None, rep=None, pf=None, bias=None, bitmask=None, out_dtype=np.float16):
    """logits [m][ld]; pasts: one id list per row; bitmask uint32 [1 or m][words]."""
    logits = np.asarray(logits)
    m = logits.shape[0]
    rows = []
    for r in range(m):
        bm = None if bitmask is None else np.asarray(bitmask)[r if np.asarray(bitmask).shape[0] > 1 else 0]
        rows.append(process_row(logits[r], size, () if pasts is None else pasts[r], rep, pf, bias, bm, out_dtype))
    return np.stack(rows)


def same_bits(a, b):
    """Equal bit for bit, a NaN standing for any NaN (the payload of a NaN is not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))
