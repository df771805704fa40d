"""The streaming waves' shares of a rectangle are cut in WHOLE SIMD ROWS (exl3_pstep.hip: wave_partition, through exl3_pstep_plan_tiles, no GPU).  A SIMD hosts streaming
waves w, w + 4, w + 8; the streaming phase is VALU-bound per SIMD and ends when the fullest SIMD ends, so every weighted rectangle gives each of the four waves of an age
group the same run (e = 0 in pX = n << 2 | e) and the four SIMDs the same number of units.  The shares are kept per op kind (gate|up and a model's other rectangles, down,
lm_head); EXL3_HIP_PSTEP_SHARES sets all kinds, EXL3_HIP_PSTEP_SHARES_DOWN / _HEAD one each."""
import ctypes
import os
import numpy as np
import pytest
from test_pstep_plan import _wave_runs, _check_wave_shares

# (hidden, inter, heads_q, heads_kv, head_dim, vocab): the bench shapes; the 70B shape is one rank's shards under TP = 8
L8B = (4096, 14336, 32, 8, 128, 128256)
L1B = (2048, 8192, 32, 8, 64, 128256)
L70B_RANK = (8192, 3584, 8, 1, 128, 16128)
CASES = [("llama-3.1-8b", L8B, 256), ("llama-3.2-1b", L1B, 256), ("llama-3.1-70b-tp8-rank", L70B_RANK, 256), ("llama-3.1-8b", L8B, 128), ("llama-3.1-8b", L8B, 64)]
ENV = ("EXL3_HIP_PSTEP_SHARES", "EXL3_HIP_PSTEP_SHARES_DOWN", "EXL3_HIP_PSTEP_SHARES_HEAD")


def _plan(shape, ncu, kind):
    """Active rectangles of one op kind, or None where the planner has no plan for that chip (small chips: test_pstep_plan.py lists the legitimate refusals)."""
    from exllamav3_amd import _lib
    tiles = np.zeros((ncu, 12), dtype=np.int32); S = ctypes.c_int(0)
    if _lib.lib().exl3_pstep_plan_tiles(*shape, ncu, kind, tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(S)) != 0:
        return None
    return tiles[tiles[:, 0] >= 0]


@pytest.fixture
def shares_env():
    """Set the shares' environment variables for one test; the planner reads them at every plan."""
    saved = {k: os.environ.pop(k, None) for k in ENV}

    def set_(**kw):
        for k in ENV: os.environ.pop(k, None)
        for k, v in kw.items(): os.environ[{"all": ENV[0], "down": ENV[1], "head": ENV[2]}[k]] = v
    yield set_
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None: os.environ[k] = v


def _per_wave(t):
    return tuple(int(p) >> 2 for p in t[9:12])


@pytest.mark.parametrize("name,shape,ncu", CASES, ids=["%s-%dcu" % (c[0], c[2]) for c in CASES])
def test_weighted_rectangles_are_cut_in_whole_simd_rows(shares_env, name, shape, ncu):
    shares_env()
    planned = 0
    for kind in range(5):
        act = _plan(shape, ncu, kind)
        if act is None:
            assert ncu < 256
            continue
        planned += 1
        for t in act:
            T, H, shares = 4 * int(t[4]) * int(t[2]), 4 * int(t[4]), tuple(int(p) for p in t[9:12])
            _check_wave_shares(T, H, shares, head=(kind == 4))              # (what the kernel assumes of any cut: test_pstep_plan.py)
            if not any(shares): continue
            assert all(p & 3 == 0 for p in shares), (kind, shares)
            runs = _wave_runs(T, shares)
            simd = [sum(u1 - u0 for w, (u0, u1) in enumerate(runs) if w % 4 == s_) for s_ in range(4)]
            assert simd == [T // 4] * 4, (kind, T, shares, simd)
            a, b, c = _per_wave(t)
            assert a >= b >= c >= 3 and a > c and a + b + c == T // 4
    assert planned >= 3


def test_kinds_weighted_before_stay_weighted_with_the_hand_worked_cuts(shares_env):
    """Llama-3.1-8B on 256 CUs.  At 460 : 370 : 170 (the shares of every kind before they were kept per kind; still down's and the lm_head's) -- gate|up: T = 112, 28 units
    per SIMD, 19 behind the three every wave decodes ahead: 3 + 19 x (.46, .37, .17) = (11.74, 10.03, 6.23) -> (12, 10, 6).  down: T = 56, 14 per SIMD, 5 behind:
    3 + 5 x (.46, .37, .17) = (5.30, 4.85, 3.85) -> (5, 5, 4).  (Group totals rounded freely were (47, 40, 25) and (21, 19, 16): 29 / 28 / 28 / 27 and 15 / 14 / 14 / 13
    units per SIMD.)  At gate|up's own default 474 : 421 : 105: 3 + 19 x (.474, .421, .105) = (12.006, 10.999, 4.995) -> (12, 11, 5)."""
    shares_env(all="460,370")
    assert {(4 * int(t[4]) * int(t[2]), _per_wave(t)) for t in _plan(L8B, 256, 2)} == {(112, (12, 10, 6))}
    assert {(4 * int(t[4]) * int(t[2]), _per_wave(t)) for t in _plan(L8B, 256, 3)} == {(56, (5, 5, 4))}
    shares_env()
    gu, dn, hd = _plan(L8B, 256, 2), _plan(L8B, 256, 3), _plan(L8B, 256, 4)
    assert len(gu) == 256 and len(dn) == 256
    assert {(4 * int(t[4]) * int(t[2]), _per_wave(t)) for t in gu} == {(112, (12, 11, 5))}
    assert {(4 * int(t[4]) * int(t[2]), _per_wave(t)) for t in dn} == {(56, (5, 5, 4))}
    assert (hd[:, 9:12] != 0).all()                                          # every lm_head rectangle (384 or 512 units) is weighted
    for t in hd:
        q, (a, b, c) = int(t[4]) * int(t[2]), _per_wave(t)
        want = [3 + (q - 9) * f / 1000.0 for f in (460, 370, 170)]
        assert a + b + c == q and max(abs(a - want[0]), abs(b - want[1]), abs(c - want[2])) < 1.0
    for kind in (0, 1):                                                      # all units decoded ahead: uniform, as before
        assert not (_plan(L8B, 256, kind)[:, 9:12] != 0).any()


def test_a_refused_nearest_triple_moves_to_a_neighbour_not_to_uniform(shares_env):
    """8B gate|up (columns of 16 units, 28 per SIMD) at 800 : 150 : 50 asks for 3 + 19 x (.80, .15, .05) = (18.2, 5.85, 3.95): the nearest triple (18, 6, 4) has runs
    longer than a column and is refused (a wave keeps two partial rows).  The cut moves to the nearest triple the kernel can take -- 16 units for the oldest group --
    and stays a weighted whole-row cut."""
    shares_env(all="800,150")
    gu = _plan(L8B, 256, 2)
    for t in gu:
        a, b, c = _per_wave(t)
        assert a == 16 == 4 * int(t[4]) and b >= c >= 3 and a + b + c == int(t[4]) * int(t[2]) and all(int(p) & 3 == 0 for p in t[9:12])
        _check_wave_shares(4 * int(t[4]) * int(t[2]), 4 * int(t[4]), tuple(int(p) for p in t[9:12]))


def test_environment_overrides_change_only_their_own_kind(shares_env):
    shares_env()
    base = {k: _plan(L8B, 256, k)[:, 9:12].copy() for k in (2, 3, 4)}
    shares_env(down="600,300")
    got = {k: _plan(L8B, 256, k)[:, 9:12].copy() for k in (2, 3, 4)}
    assert np.array_equal(got[2], base[2]) and np.array_equal(got[4], base[4]) and not np.array_equal(got[3], base[3])
    shares_env(head="400,350")
    got = {k: _plan(L8B, 256, k)[:, 9:12].copy() for k in (2, 3, 4)}
    assert np.array_equal(got[2], base[2]) and np.array_equal(got[3], base[3]) and not np.array_equal(got[4], base[4])
    # one kind uniform, the others untouched
    shares_env(down="0,0")
    got = {k: _plan(L8B, 256, k)[:, 9:12].copy() for k in (2, 3, 4)}
    assert not got[3].any() and np.array_equal(got[2], base[2]) and np.array_equal(got[4], base[4])
    # the general variable still means every kind, and a kind's own variable wins over it
    shares_env(all="0,0")
    assert not any(_plan(L8B, 256, k)[:, 9:12].any() for k in range(5))
    shares_env(all="0,0", head="460,370")
    got = {k: _plan(L8B, 256, k)[:, 9:12].copy() for k in (2, 3, 4)}
    assert not got[2].any() and not got[3].any() and np.array_equal(got[4], base[4])
    shares_env(all="400,350")
    got = {k: _plan(L8B, 256, k)[:, 9:12].copy() for k in (2, 3, 4)}
    assert all(not np.array_equal(got[k], base[k]) for k in (2, 4))
