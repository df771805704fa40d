"""Hand-worked cases of the numpy references of speculative decoding (tests/_spec_ref.py): the n-gram drafter and the accept rule.  CPU only."""
import numpy as np
import _spec_ref as R


def test_ngram_suffix_of_period_one_shrinks_the_draft():
    # aaaa: the suffix aaa also ends at e = 3, one token before the end -- only L - e = 1 token lies behind it
    assert R.ngram_draft([7, 7, 7, 7], 4, 3, 2, 8) == [7]
    assert R.ngram_draft([7, 7, 7, 7], 4, 3, 1, 1) == [7]
    assert R.ngram_draft([7, 7, 7, 7, 7, 7], 6, 2, 2, 3) == [7]            # match_max 3: the suffix of 3 ends at e = 5 at the latest


def test_ngram_match_only_at_the_very_start():
    assert R.ngram_draft([1, 2, 3, 4, 5, 1, 2], 7, 3, 2, 8) == [3, 4, 5]
    assert R.ngram_draft([1, 2, 3, 4, 5, 1, 2], 7, 2, 2, 8) == [3, 4]
    assert R.ngram_draft([1, 2, 3, 4, 5, 1, 2], 7, 3, 3, 8) == []           # no match of 3


def test_ngram_two_matches_of_equal_length_the_later_wins():
    assert R.ngram_draft([1, 2, 9, 1, 2, 8, 1, 2], 8, 3, 2, 8) == [8, 1, 2]
    assert R.ngram_draft([1, 2, 9, 1, 2, 8, 1, 2], 8, 1, 2, 8) == [8]


def test_ngram_a_longer_match_wins_over_a_later_shorter_one():
    h = [5, 1, 2, 3, 9, 2, 3, 7, 1, 2, 3]
    assert R.ngram_draft(h, 11, 3, 2, 8) == [9, 2, 3]                       # 1 2 3 at e = 4 beats 2 3 at e = 7
    assert R.ngram_draft(h, 11, 3, 2, 2) == [7, 1, 2]                       # capped at 2 tokens the later one is found
    assert R.ngram_draft(h, 11, 3, 4, 8) == []


def test_ngram_history_not_longer_than_match_min_gives_no_draft():
    assert R.ngram_draft([4], 1, 3, 1, 8) == []
    assert R.ngram_draft([4, 4], 2, 3, 2, 8) == []
    assert R.ngram_draft([4, 4], 2, 3, 1, 8) == [4]
    assert R.ngram_draft([4, 4, 4], 3, 3, 2, 8) == [4]
    # positions behind L are not part of the history
    assert R.ngram_draft([1, 2, 3, 1, 2, 3], 3, 3, 1, 8) == []


def test_script_draft_stops_at_the_first_entry_that_is_no_id():
    s = [-1, -1, 5, 6, -1, 8, 2000, 9]
    assert R.script_draft(s, 2, 3, 1024) == [5, 6]
    assert R.script_draft(s, 2, 1, 1024) == [5]
    assert R.script_draft(s, 4, 3, 1024) == []
    assert R.script_draft(s, 5, 3, 1024) == [8]                             # 2000 lies outside the vocabulary
    assert R.script_draft(s, 7, 3, 1024) == [9]                             # the table ends


def _state(base, produced, nd):
    s = np.zeros(R.STATE_WORDS, dtype=np.int64)
    s[R.BASE], s[R.PRODUCED], s[R.NDRAFT], s[R.LIVE] = base, produced, nd, 1
    return s


def _run(sampled, stop=(), max_new=16, produced=0, nd=3, in_tokens=(10, 11, 12, 13)):
    hist = np.full(32, -1); hist[:5] = [1, 2, 3, 4, 10]
    out = np.full(max_new, -1)
    return R.accept(sampled, in_tokens, _state(4, produced, nd), 6, hist, out, max_new, 1024, stop)


def test_accept_none_partial_all():
    st, rnd, hist, out = _run([20, 21, 22, 23])
    assert (st[R.BASE], st[R.PRODUCED], st[R.ACCEPTED], st[R.DRAFTED], st[R.ROUNDS], st[R.LIVE], rnd) == (5, 1, 0, 3, 1, 1, 7)
    assert hist[5] == 20 and hist[6] == -1 and out[0] == 20 and out[1] == -1
    st, rnd, hist, out = _run([11, 12, 99, 50])
    assert (st[R.BASE], st[R.PRODUCED], st[R.ACCEPTED]) == (7, 3, 2)
    assert hist[5:9].tolist() == [11, 12, 99, -1] and out[:4].tolist() == [11, 12, 99, -1]
    st, rnd, hist, out = _run([11, 12, 13, 14])
    assert (st[R.BASE], st[R.PRODUCED], st[R.ACCEPTED]) == (8, 4, 3)
    assert hist[5:10].tolist() == [11, 12, 13, 14, -1] and out[:5].tolist() == [11, 12, 13, 14, -1]
    # padding behind n_draft is never taken for a draft, even where it equals the sample
    st, _, hist, _ = _run([11, 10, 10, 10], nd=1, in_tokens=(10, 11, 10, 10))
    assert (st[R.BASE], st[R.ACCEPTED], st[R.DRAFTED]) == (6, 1, 1) and hist[5:8].tolist() == [11, 10, -1]


def test_accept_stop_id_in_the_middle_is_kept_and_ends_the_row():
    st, rnd, hist, out = _run([11, 12, 13, 14], stop=(12, 500))
    assert (st[R.BASE], st[R.PRODUCED], st[R.ACCEPTED], st[R.DONE], st[R.LIVE]) == (6, 2, 1, 1, 0)
    assert hist[5:8].tolist() == [11, 12, -1] and out[:3].tolist() == [11, 12, -1]
    # frozen: only the round word moves
    st2, rnd2, hist2, out2 = R.accept([1, 2, 3, 4], (10, 1, 2, 3), st, rnd, hist, out, 16, 1024, (12, 500))
    assert rnd2 == rnd + 1 and st2.tolist() == st.tolist() and hist2.tolist() == hist.tolist() and out2.tolist() == out.tolist()


def test_accept_budget_cut_on_the_last_round():
    st, rnd, hist, out = _run([11, 12, 13, 14], max_new=10, produced=8)
    assert (st[R.BASE], st[R.PRODUCED], st[R.ACCEPTED], st[R.LIVE], st[R.DONE]) == (6, 10, 1, 0, 0)
    assert hist[5:8].tolist() == [11, 12, -1] and out[8:].tolist() == [11, 12]


def test_accept_sample_outside_the_vocabulary_freezes_the_row():
    st, rnd, hist, out = _run([11, -1, 13, 14])
    assert (st[R.BASE], st[R.PRODUCED], st[R.INVALID], st[R.LIVE]) == (5, 1, 1, 0) and hist[5:7].tolist() == [11, -1]
    st, _, hist, _ = _run([1024, 0, 0, 0])
    assert (st[R.BASE], st[R.PRODUCED], st[R.INVALID], st[R.LIVE]) == (4, 0, 1, 0) and hist[5] == -1
    # an unconsumed row may hold anything
    st, _, _, _ = _run([20, -1, -1, -1])
    assert (st[R.BASE], st[R.INVALID], st[R.LIVE]) == (5, 0, 1)


def test_feed_pads_with_the_committed_token():
    hist = [1, 2, 9, 1, 2, 8, 1, 2] + [-1] * 8
    toks, nd, pos, lens = R.feed(hist, _state(7, 0, 0), 5, 4, 16, 1024)
    assert toks == [2, 8, 1, 2, 2] and nd == 3 and pos == [7, 8, 9, 10, 11] and lens == [8, 9, 10, 11, 12]
    toks, nd, _, _ = R.feed(hist, _state(7, 0, 0), 3, 2, 16, 1024, script=[-1] * 8 + [40, -1, 41] + [-1] * 5)
    assert toks == [2, 40, 2] and nd == 1
    s = _state(7, 16, 0)
    assert R.feed(hist, s, 3, 2, 16, 1024) is None
