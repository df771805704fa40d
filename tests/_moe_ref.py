"""CPU restatement (numpy / plain Python) of the two integer contracts of the MoE dispatch (csrc/exl3_routing.hip, the comment block above
moe_build_slots_kernel, and ext.moe_scatter's docstring).  Not a port of the kernels: no prefix-sum tables, no workgroup loops -- one walk over the
experts in order, and a per-token sum in float64.

The assignments (token, expert) of a batch arrive GROUPED BY EXPERT: token_sorted[p] is the token of assignment p, expert 0's assignments first
(expert_count[0] of them), then expert 1's, and so on -- refused experts keep their place in that list."""
import numpy as np


def build_slots(expert_count, token_sorted, max_rows, m, ns_max):
    """-> (slot_expert int64 [ns_max], slot_tok int64 [ns_max * m], rowmap int32 [T]).
    Accepted experts: 0 < count <= max_rows.  An accepted expert's assignments are cut into chunks of m consecutive ones, one chunk per slot; its
    first slot is the exclusive prefix sum of ceil(count / m) over the accepted experts before it.  Row r of a slot carries the token of the chunk's
    r-th assignment, rows past the chunk's end repeat its last assignment.  Unused slots: expert -1, token 0.  rowmap[p] = slot * m + row of an
    accepted assignment p, -1 for the assignments of refused experts."""
    expert_count = [int(c) for c in expert_count]
    token_sorted = [int(t) for t in token_sorted]
    T = len(token_sorted)
    assert sum(expert_count) == T, "expert_count must add up to the number of assignments"
    slot_expert = np.full((ns_max,), -1, dtype=np.int64)
    slot_tok = np.zeros((ns_max, m), dtype=np.int64)
    rowmap = np.full((T,), -1, dtype=np.int32)
    first, slot = 0, 0                                      # first assignment of the expert; next free slot
    for e, c in enumerate(expert_count):
        if 0 < c <= max_rows:
            for lo in range(first, first + c, m):
                chunk = list(range(lo, min(lo + m, first + c)))
                assert slot < ns_max, "more slots than ns_max"
                slot_expert[slot] = e
                for r in range(m):
                    slot_tok[slot, r] = token_sorted[chunk[min(r, len(chunk) - 1)]]
                for r, p in enumerate(chunk):
                    rowmap[p] = slot * m + r
                slot += 1
        first += c
    return slot_expert, slot_tok.reshape(-1), rowmap


def ns_max(E, T, m):
    """The slot count exl3_moe allocates: every expert with rows has at most one partly filled slot, the rest are full."""
    return min(E, T) + T // m


def scatter(D, rowmap, token_sorted, weight_sorted, out):
    """-> float64 [tokens, hidden]: out[t] + sum over token t's assignments p with rowmap[p] >= 0, in ascending p, of weight_sorted[p] * D[rowmap[p]]."""
    D = np.asarray(D, dtype=np.float64)
    w = np.asarray(weight_sorted).astype(np.float64)
    res = np.array(out, dtype=np.float64)
    for p in range(len(token_sorted)):                      # ascending p over all tokens = ascending p per token
        if rowmap[p] >= 0:
            res[int(token_sorted[p])] += w[p] * D[int(rowmap[p])]
    return res


def scatter_abs(D, rowmap, token_sorted, weight_sorted, out):
    """-> (float64 [tokens, hidden] = |out| + sum |w * d| over the same terms, int [tokens] = the number of terms): the scale of a summation-error bound."""
    D = np.abs(np.asarray(D, dtype=np.float64))
    w = np.abs(np.asarray(weight_sorted).astype(np.float64))
    res = np.abs(np.array(out, dtype=np.float64))
    n = np.zeros((res.shape[0],), dtype=np.int64)
    for p in range(len(token_sorted)):
        if rowmap[p] >= 0:
            res[int(token_sorted[p])] += w[p] * D[int(rowmap[p])]
            n[int(token_sorted[p])] += 1
    return res, n
