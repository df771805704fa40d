"""Test-only restatement of the EXL3 trellis encoder (the reference's quantize_tiles: exllamav3_ext/quant/quantize.cu:27-87,
quant/quantize_tiles_kernel.cuh:19-298), vectorised over tiles in numpy.  The product code never imports this module.

Every fp16 operation of the kernel (sub, mul, fma) is evaluated in float64 and rounded once to float16: at these magnitudes the float64 value is
exact or too far below half an fp16 ulp to matter, so this reproduces round-to-nearest fp16 arithmetic."""
from __future__ import annotations
import numpy as np

from oracle import exl3_oracle as orc

F16_INF = np.float64(np.inf)


def _f16(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return x.astype(np.float16).astype(np.float64)


_DEC = {}


def decoded_states(cb: int) -> np.ndarray:
    """decode(s) for all 65536 states, float64 of the fp16 values."""
    if cb not in _DEC:
        _DEC[cb] = orc.decode(np.arange(65536, dtype=np.uint16), cb).astype(np.float64)
    return _DEC[cb]


def bitrev5(x):
    x = np.asarray(x)
    r = np.zeros_like(x)
    for b in range(5):
        r |= ((x >> b) & 1) << (4 - b)
    return r


def argmin_key_order(costs: np.ndarray) -> np.ndarray:
    """argmin over the last axis with the reference's tie order: (cost, bitrev5(s), bitrev5(l), e) with v = e mod 1024,
    s = 16 (v >> 9) + ((v >> 5) & 15), l = v & 31."""
    E = costs.shape[-1]
    e = np.arange(E)
    v = e & 1023
    s = 16 * (v >> 9) + ((v >> 5) & 15)
    l = v & 31
    order = np.lexsort((e, bitrev5(l), bitrev5(s)))                      # tie order of the leaves, cost aside
    c = costs[..., order]
    return order[np.argmin(c, axis=-1)]                                  # first minimal leaf in that order


def argmin_shuffle_tree(costs: np.ndarray) -> int:
    """Literal restatement of the reference's reduction (quantize_tiles_kernel.cuh:219-268) for one cost vector: 512 threads x two strided
    halves, a __shfl_down tree over the 32 lanes of each warp, then the same tree over the 32 per-half-warp slots.  A node keeps its own value
    unless the other is strictly less."""
    E = costs.shape[0]
    NT = 512
    lmin = np.full((2, NT), np.inf)
    lidx = np.full((2, NT), -1, dtype=np.int64)
    for h in range(2):
        for t in range(NT):
            for e in range(t + h * NT, E, 2 * NT):
                if costs[e] < lmin[h, t]:
                    lmin[h, t], lidx[h, t] = costs[e], e

    def tree(vals, idxs):
        vals, idxs = list(vals), list(idxs)
        off = 16
        while off > 0:
            nv, ni = list(vals), list(idxs)
            for lane in range(32):
                src = lane + off
                if src < 32:                                             # (out-of-range lanes read their own value: no change)
                    if vals[src] < vals[lane]:
                        nv[lane], ni[lane] = vals[src], idxs[src]
            vals, idxs = nv, ni
            off >>= 1
        return vals[0], idxs[0]

    slot_v = np.full(32, np.inf)
    slot_i = np.full(32, -1, dtype=np.int64)
    for w in range(16):
        for h in range(2):
            lanes = slice(32 * w, 32 * w + 32)
            v, i = tree(lmin[h, lanes], lidx[h, lanes])
            slot_v[16 * h + w], slot_i[16 * h + w] = v, i
    return int(tree(slot_v, slot_i)[1])


def _candidates(K: int):
    E = 65536 >> K
    s = np.arange(65536).reshape(1 << K, E)                              # s[k, e] = (k << (16 - K)) | e
    return s, s >> K                                                     # state, predecessor node


def _forward(w: np.ndarray, K: int, cb: int, roll: int, pre: np.ndarray | None):
    """One pass over positions roll, roll+1, ... (mod 256).  w (n, 256) float64 of fp16.  Returns (final costs (n, E), bp (n, 256, E))."""
    n = w.shape[0]
    E = 65536 >> K
    s, pred = _candidates(K)
    dec = decoded_states(cb)[s]                                          # (2^K, E)
    bp = np.empty((n, 256, E), dtype=np.int32)
    cost = None
    rows = np.arange(n)[:, None]
    for step in range(256):
        t = (step + roll) & 255
        delta = _f16(dec[None] - w[:, t, None, None])                    # (n, 2^K, E)
        if step == 0:
            c = _f16(delta * delta)
            if pre is not None:
                c = np.where(pred[None] == pre[:, None, None], c, F16_INF)
        else:
            c = _f16(delta * delta + cost[rows[:, :, None], pred[None]])
        k = np.argmin(c, axis=1)                                         # first minimum: strictly-less update in increasing k
        cost = np.take_along_axis(c, k[:, None, :], axis=1)[:, 0, :]
        bp[:, t, :] = pred[k, np.arange(E)[None, :]]
    return cost, bp


def quantize_tiles(tiles: np.ndarray, K: int, cb: int):
    """tiles (n, 256) float32 -> (out (n, 256) float32, idx (n, 256) uint16), bit-identical to the reference encoder."""
    tiles = np.asarray(tiles, dtype=np.float32)
    n = tiles.shape[0]
    w = tiles.astype(np.float16).astype(np.float64)
    rows = np.arange(n)
    # pass A: positions 128 .. 255, 0 .. 127, unconstrained; trace back from the argmin through position 0
    cost, bp = _forward(w, K, cb, 128, None)
    e = argmin_key_order(cost)
    for t in range(127, -1, -1):
        e = bp[rows, t, e]
    pre = e
    # pass B: positions 0 .. 255 with the predecessor of position 0 fixed; tail-biting trace back from node pre at position 255
    _, bp = _forward(w, K, cb, 0, pre)
    idx = np.empty((n, 256), dtype=np.uint16)
    e = pre.copy()
    for t in range(255, -1, -1):
        p = bp[rows, t, e]
        idx[:, t] = (p << K) | e
        e = p
    out = decoded_states(cb)[idx].astype(np.float32)
    return out, idx


def viterbi_f64_constrained(tiles: np.ndarray, K: int, cb: int, pre: np.ndarray) -> np.ndarray:
    """Textbook float64 Viterbi (no rounding): the least squared error of a path whose position-0 predecessor is pre[i] and whose node at
    position 255 is pre[i] (a tail-biting path through pre)."""
    w = np.asarray(tiles, dtype=np.float32).astype(np.float16).astype(np.float64)
    n = w.shape[0]
    s, pred = _candidates(K)
    dec = decoded_states(cb)[s]
    rows = np.arange(n)[:, None]
    cost = None
    for t in range(256):
        d2 = (dec[None] - w[:, t, None, None]) ** 2
        if t == 0:
            c = np.where(pred[None] == pre[:, None, None], d2, np.inf)
        else:
            c = d2 + cost[rows[:, :, None], pred[None]]
        cost = c.min(axis=1)
    return cost[np.arange(n), pre]


def is_tailbiting(idx: np.ndarray, K: int) -> np.ndarray:
    E = 65536 >> K
    idx = idx.astype(np.int64)
    chain = np.all((idx[:, 1:] >> K) == (idx[:, :-1] & (E - 1)), axis=1)
    return chain & ((idx[:, 0] >> K) == (idx[:, 255] & (E - 1)))
