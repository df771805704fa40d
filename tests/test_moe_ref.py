"""CPU checks of the MoE dispatch contracts' restatement (tests/_moe_ref.py): a hand-worked slot list, the invariants of build_slots on random ragged
counts, and scatter against a dense weighted sum.  tests/test_gpu_moe_wide.py holds the kernels against this restatement."""
import numpy as np
import pytest

import _moe_ref as R


def _ragged(rng, E, T, idle=0.3):
    """Random counts adding up to T with about `idle` of the experts idle, and a token for every assignment."""
    p = rng.random(E) * (rng.random(E) >= idle)
    if p.sum() == 0:
        p[rng.integers(E)] = 1.0
    counts = rng.multinomial(T, p / p.sum())
    return counts.astype(np.int64), rng.integers(0, max(1, T // 3), T).astype(np.int64)


def test_build_slots_hand_worked_example():
    """5 experts, m = 2, max_rows = 3: expert 0 (3 rows) fills slots 0 and 1, expert 1 is idle, expert 2 (4 rows) is refused, expert 3 (1 row) gets slot 2,
    expert 4 (2 rows) slot 3; ns_max = min(5, 10) + 10 // 2 = 10 slots, 6 of them unused."""
    counts = [3, 0, 4, 1, 2]
    toks = [10, 11, 12, 20, 21, 22, 23, 30, 40, 41]
    se, st, rm = R.build_slots(counts, toks, 3, 2, R.ns_max(5, 10, 2))
    assert se.dtype == np.int64 and st.dtype == np.int64 and rm.dtype == np.int32
    assert se.tolist() == [0, 0, 3, 4] + [-1] * 6
    assert st.reshape(-1, 2).tolist() == [[10, 11], [12, 12], [30, 30], [40, 41]] + [[0, 0]] * 6
    assert rm.tolist() == [0, 1, 2, -1, -1, -1, -1, 4, 6, 7]


@pytest.mark.parametrize("E,T,m,max_rows", [(8, 16, 1, 4), (6, 48, 16, 22), (128, 192, 16, 9), (512, 4096, 4, 64), (1, 7, 4, 7), (1, 7, 4, 6), (5, 1, 1, 1),
                                            (384, 24, 3, 2), (33, 1000, 7, 40)])
def test_build_slots_invariants_on_ragged_counts(E, T, m, max_rows):
    for seed in range(4):
        rng = np.random.default_rng([E, T, m, seed])
        counts, toks = _ragged(rng, E, T)
        nsm = R.ns_max(E, T, m)
        se, st, rm = R.build_slots(counts, toks, max_rows, m, nsm)
        st = st.reshape(nsm, m)
        start = np.concatenate([[0], np.cumsum(counts)])
        expert_of = np.repeat(np.arange(E), counts)
        accepted = (counts > 0) & (counts <= max_rows)
        used = int((se >= 0).sum())
        # the used slots are a prefix, in ascending expert order; their number is the chunk count and stays within ns_max
        assert (se[:used] >= 0).all() and (se[used:] == -1).all() and (np.diff(se[:used]) >= 0).all()
        assert used == int(np.ceil(counts[accepted] / m).sum()) <= nsm
        assert (st[used:] == 0).all()
        # every accepted assignment sits in exactly one (slot, row) pair, that pair belongs to its expert and carries its token
        acc_p = np.flatnonzero(accepted[expert_of])
        assert len(set(rm[acc_p].tolist())) == len(acc_p) and (rm[acc_p] >= 0).all() and (rm[acc_p] < used * m).all()
        assert (se[rm[acc_p] // m] == expert_of[acc_p]).all()
        assert (st.reshape(-1)[rm[acc_p]] == toks[acc_p]).all()
        # refused experts touch nothing: no rowmap entry, no slot
        assert (rm[np.flatnonzero(~accepted[expert_of])] == -1).all()
        assert not np.isin(se[:used], np.flatnonzero(~accepted)).any()
        # no slot mixes experts: every row of a used slot -- the padded ones too -- is a token of an assignment of the slot's expert, the rows that no rowmap
        # entry points at repeat the slot's last mapped row, and an expert's slots start at the prefix sum of the chunk counts before it
        mapped = np.zeros((nsm * m,), dtype=bool); mapped[rm[acc_p]] = True
        mapped = mapped.reshape(nsm, m)
        base = 0
        for e in np.flatnonzero(accepted):
            mine = np.flatnonzero(se == e)
            assert mine.tolist() == list(range(base, base + -(-int(counts[e]) // m)))
            base += len(mine)
            for i, j in enumerate(mine):
                n = int(mapped[j].sum())
                assert n == min(m, counts[e] - i * m) and mapped[j, :n].all()
                assert st[j, :n].tolist() == toks[start[e] + i * m: start[e] + i * m + n].tolist()
                assert (st[j, n:] == st[j, n - 1]).all()


def test_build_slots_rejects_inconsistent_counts():
    with pytest.raises(AssertionError):
        R.build_slots([2, 2], [0, 1, 2], 4, 2, 4)


def test_scatter_matches_a_dense_weighted_sum_and_skips_unmapped_assignments():
    rng = np.random.default_rng(0)
    tokens, hidden, T, rows = 7, 12, 60, 80
    D = rng.standard_normal((rows, hidden)).astype(np.float32)
    rm = rng.permutation(rows)[:T].astype(np.int32)
    rm[rng.random(T) < 0.25] = -1
    tok = rng.integers(0, tokens - 1, T).astype(np.int64)                   # the last token has no assignment
    w = rng.uniform(-1, 1, T).astype(np.float16)
    out0 = rng.standard_normal((tokens, hidden)).astype(np.float32)
    got = R.scatter(D, rm, tok, w, out0)
    assert got.dtype == np.float64
    M = np.zeros((tokens, rows))                                            # M[t, row] = weight of the assignment that maps token t to that row
    for p in range(T):
        if rm[p] >= 0:
            M[tok[p], rm[p]] += float(w[p])
    assert np.allclose(got, out0.astype(np.float64) + M @ D.astype(np.float64), rtol=1e-12, atol=1e-12)
    assert np.array_equal(got[tokens - 1], out0[tokens - 1].astype(np.float64))
    mag, n = R.scatter_abs(D, rm, tok, w, out0)
    assert np.allclose(mag, np.abs(out0) + np.abs(M) @ np.abs(D.astype(np.float64)), rtol=1e-12, atol=1e-12)
    assert n.tolist() == [int(((tok == t) & (rm >= 0)).sum()) for t in range(tokens)]
    assert (np.abs(got) <= mag + 1e-12).all()
