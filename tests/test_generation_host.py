"""The host side of generate() (exllamav3_amd/generation.py) without a GPU: when the live word is read, what the stop arguments mean, how stop tokens and EOS cut
one sequence versus a batch.  Every expected value is written out by hand."""
import pytest
import torch
from exllamav3_amd.generation import finish_tokens, parse_stop, replay_loop


def drive(n, every, live_from=None):
    """replay_loop with a counting replay and a live word that reads 0 once `live_from` replays have run (None: never).  Returns the result and the replay counts
    at which the live word was read."""
    count, reads = [0], []

    def replay():
        count[0] += 1

    def read_live():
        reads.append(count[0])
        return 0 if live_from is not None and count[0] >= live_from else 1

    out = replay_loop(replay, n, every, read_live)
    assert count[0] == out[0]
    return out, reads


def test_replay_loop_polls_every_nth_replay_but_never_behind_the_last():
    assert drive(0, 4) == ((0, 0, None), [])
    assert drive(1, 1) == ((1, 0, None), [])
    assert drive(16, 4) == ((16, 3, None), [4, 8, 12])
    assert drive(17, 8) == ((17, 2, None), [8, 16])


def test_replay_loop_leaves_at_the_first_poll_that_reads_zero():
    assert drive(16, 4, live_from=5) == ((8, 2, 8), [4, 8])


def test_replay_loop_without_an_interval_never_reads():
    def read_live():
        raise AssertionError("read_live called without an interval")
    done = []
    assert replay_loop(lambda: done.append(1), 16, None, read_live) == (16, 0, None)
    assert len(done) == 16


def test_stop_arguments():
    with pytest.raises(ValueError):
        parse_stop([], None)
    with pytest.raises(ValueError):
        parse_stop(list(range(65)), None)
    with pytest.raises(ValueError):
        parse_stop([7], 0)
    with pytest.raises(ValueError):
        parse_stop(None, 4)                                     # the plain path: an interval needs ids
    with pytest.raises(ValueError):
        parse_stop([], None, always_poll=True)
    with pytest.raises(ValueError):
        parse_stop(None, 0, always_poll=True)
    assert parse_stop(None, None) == (None, None)               # the plain path: no ids, no polling
    assert parse_stop(None, None, always_poll=True) == (None, 16)
    assert parse_stop(None, 4, always_poll=True) == (None, 4)
    assert parse_stop([7, 3], None) == ([7, 3], 16)
    assert parse_stop(torch.tensor([7, 3]), 5) == ([7, 3], 5)
    assert parse_stop(list(range(64)), 1, always_poll=True) == (list(range(64)), 1)


def test_stop_tokens_cut_one_sequence_and_fill_a_batch():
    got = finish_tokens([[5, 7, 9, 7]], True, [7, 3])
    assert got.dtype == torch.int64 and got.tolist() == [5, 7]
    got = finish_tokens([[5, 7, 9, 7], [1, 2, 3, 4]], False, [7, 3])
    assert got.dtype == torch.int64 and got.tolist() == [[5, 7, 7, 7], [1, 2, 3, 7]]     # filled with stop[0]; not trimmed
    assert finish_tokens([[5, 8, 9, 6]], True, [7, 3]).tolist() == [5, 8, 9, 6]
    assert finish_tokens([[5, 8, 9, 6], [1, 2, 4, 4]], False, [7, 3]).tolist() == [[5, 8, 9, 6], [1, 2, 4, 4]]


def test_eos_cuts_one_sequence_and_fills_a_batch():
    got = finish_tokens([[4, 6, 8]], True, None, 6)
    assert got.dtype == torch.int64 and got.tolist() == [4, 6]
    got = finish_tokens([[4, 6, 8], [1, 2, 3]], False, None, 6)
    assert got.dtype == torch.int64 and got.tolist() == [[4, 6, 6], [1, 2, 3]]
    assert finish_tokens([[4, 5, 8]], True, None, 6).tolist() == [4, 5, 8]
    assert finish_tokens([[4, 5, 8], [1, 2, 3]], False, None, 6).tolist() == [[4, 5, 8], [1, 2, 3]]


def test_finishing_takes_int32_rows_and_applies_eos_behind_the_stop_cut():
    got = finish_tokens(torch.tensor([[5, 6, 7, 9]], dtype=torch.int32), True, [7], 6)
    assert got.dtype == torch.int64 and got.tolist() == [5, 6]
    got = finish_tokens(torch.tensor([[5, 9, 7, 6], [6, 1, 2, 3]], dtype=torch.int32), False, [7], 6)
    assert got.dtype == torch.int64 and got.tolist() == [[5, 9, 7, 7], [6, 6, 6, 6]]
    assert finish_tokens(torch.empty((1, 0), dtype=torch.int32), True, None, 6).tolist() == []
