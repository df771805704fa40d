"""CPU restatement (numpy) of the device sampler's contract (include/exl3_hip.h: exl3_sample): Philox4x32-10, the uniform and the Gumbel transform, the
objective in fp64, and the kept-set definitions of modes 2 / 3 evaluated in fp64 from the fp16 logits.  Not a port of the kernel: no histograms, no radix
select -- sorts and exact cumulative sums."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32, key: 2 ints -> 4 uint32 arrays (Salmon et al., SC'11)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)
        p1 = c[2] * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in c]


def uniform(w):
    """u = ((w >> 9) + 0.5) * 2^-23: exact in fp32, strictly inside (0, 1)."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(size, row, step, seed):
    """Gumbel(0, 1) noise (fp64) of columns 0 .. size - 1 of `row` at `step` under `seed` (64-bit)."""
    step &= 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((np.arange(size, dtype=np.uint64), row, step & MASK, step >> 32), (seed & MASK, (seed >> 32) & MASK))[0]
    return -np.log(-np.log(uniform(w)))


def valid_row(l):
    """l: fp16 row (already cut to `size`)."""
    lf = l.astype(np.float64)
    return not (np.isnan(lf).any() or np.isposinf(lf).any()) and bool(np.isfinite(lf).any())


def greedy(l):
    return int(np.argmax(l.astype(np.float64))) if valid_row(l) else -1          # np.argmax: the first of equal maxima


def topk_cutoff(l, k):
    """The k-th largest finite logit counted with multiplicity (all of them when there are fewer than k)."""
    f = np.sort(l[np.isfinite(l)].astype(np.float64))[::-1]
    return float(f[min(k, f.size) - 1])


def minp_threshold(l, minp_log):
    M = np.float32(l[np.isfinite(l)].max())
    return float(np.float32(M + np.float32(minp_log)))                           # one fp32 add


def masses(l, c0, inv_temp_filter):
    """(distinct surviving values descending, mass of each class, Z) with weights exp((l - M) * inv_temp_filter) in fp64, over finite l >= c0."""
    f = l[np.isfinite(l)].astype(np.float64)
    M = f.max()
    f = f[f >= c0]
    vals, counts = np.unique(f, return_counts=True)
    vals, counts = vals[::-1], counts[::-1]
    w = counts * np.exp((vals - M) * float(np.float32(inv_temp_filter)))
    return vals, w, float(w.sum())


def topp_cutoff(l, c0, top_p, inv_temp_filter):
    """A value class stays while the mass down to and including it is <= top_p * Z; the top class always stays."""
    vals, w, Z = masses(l, c0, inv_temp_filter)
    keep = np.cumsum(w) <= float(np.float32(top_p)) * Z
    keep[0] = True
    return float(vals[keep][-1])


def cutoff(l, mode, filters=0, top_k=0, top_p=1.0, inv_temp_filter=1.0, minp_log=0.0):
    """The kept set of a valid row is { i : l_i finite and l_i >= cutoff }."""
    c = -np.inf
    if mode == 3 and filters & 1:
        c = max(c, topk_cutoff(l, top_k))
    if mode == 2 or (mode == 3 and filters & 4):
        c = max(c, minp_threshold(l, minp_log))
    if mode == 3 and filters & 2:
        c = max(c, topp_cutoff(l, c, top_p, inv_temp_filter))
    return c


def objective(l, inv_temp, row, step, seed, cut=-np.inf):
    """v_i = l_i * inv_temp + g_i in fp64 over the kept set (-inf elsewhere)."""
    lf = l.astype(np.float64)
    v = lf * float(np.float32(inv_temp)) + gumbel(l.size, row, step, seed)
    v[~(np.isfinite(lf) & (lf >= cut))] = -np.inf
    return v


def sample(l, mode, inv_temp=1.0, row=0, step=0, seed=0, **kw):
    if not valid_row(l):
        return -1
    if mode == 0:
        return greedy(l)
    return int(np.argmax(objective(l, inv_temp, row, step, seed, cutoff(l, mode, **kw))))
