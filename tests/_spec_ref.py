"""numpy / plain-Python references of the two rules of speculative decoding (include/exl3_hip.h: exl3_spec_accept, exl3_spec_draft_ngram), written from their
definitions: the n-gram drafter by brute force over every length and end position, the accept rule as a straight loop."""
import numpy as np

BASE, PRODUCED, LIVE, DONE, INVALID, NDRAFT, ROUNDS, DRAFTED, ACCEPTED = range(9)
STATE_WORDS = 9


def ngram_draft(hist, L, k, match_min, match_max):
    """Draft behind the committed history hist[0 .. L): the longest n in [match_min, match_max] with n <= L - 1 for which the suffix hist[L - n .. L) equals
    hist[e - n .. e) for some e <= L - 1; among the matches of that n the largest e; the draft is hist[e .. e + c), c = min(k, L - e).  -> list (empty: no match)."""
    hist = [int(t) for t in hist[:L]]
    for n in range(min(match_max, L - 1), match_min - 1, -1):
        suffix = hist[L - n:L]
        for e in range(L - 1, n - 1, -1):
            if hist[e - n:e] == suffix:
                return hist[e:e + min(k, L - e)]
    return []


def script_draft(script, L, k, vocab):
    """Scripted drafter: script[L .. L + c), c = the count of leading entries inside [0, vocab), at most k."""
    out = []
    while len(out) < k and L + len(out) < len(script) and 0 <= int(script[L + len(out)]) < vocab:
        out.append(int(script[L + len(out)]))
    return out


def frozen(state, max_new):
    return bool(state[DONE] or state[INVALID] or state[PRODUCED] >= max_new)


def accept(sampled, in_tokens, state, rnd, hist, tokens_out, max_new, vocab, stop_ids=()):
    """One exl3_spec_accept launch on copies: -> (state, round, hist, tokens_out)."""
    state, hist, tokens_out = np.array(state, dtype=np.int64), np.array(hist, dtype=np.int64), np.array(tokens_out, dtype=np.int64)
    rnd = int(rnd) + 1
    if frozen(state, max_new):
        state[LIVE] = 0
        return state, rnd, hist, tokens_out
    m = len(in_tokens)
    base, produced = int(state[BASE]), int(state[PRODUCED])
    nd = min(max(int(state[NDRAFT]), 0), m - 1)
    n = 0
    while n < nd and int(in_tokens[n + 1]) == int(sampled[n]):
        n += 1
    n = min(n, max_new - produced - 1)
    emitted = 0
    for i in range(n + 1):
        tok = int(sampled[i])
        if not (0 <= tok < vocab) or base + 1 + i >= len(hist):
            state[INVALID] = 1
            break
        hist[base + 1 + i] = tok
        tokens_out[produced + i] = tok
        emitted += 1
        if tok in stop_ids:
            state[DONE] = 1
            break
    state[BASE] = base + emitted
    state[PRODUCED] = produced + emitted
    state[ROUNDS] += 1
    state[DRAFTED] += nd
    state[ACCEPTED] += max(emitted - 1, 0)
    state[LIVE] = int(not frozen(state, max_new))
    return state, rnd, hist, tokens_out


def feed(hist, state, m, k, max_new, vocab, match_min=2, match_max=8, script=None):
    """What exl3_spec_draft_ngram writes for a live state: -> (in_tokens [m], n_draft, positions [m], attn_lens [m]); None when the state is frozen."""
    if frozen(state, max_new):
        return None
    base = int(state[BASE])
    L = base + 1
    d = script_draft(script, L, k, vocab) if script is not None else ngram_draft(hist, L, k, match_min, match_max)
    toks = [int(hist[base])] + d + [int(hist[base])] * (m - 1 - len(d))
    return toks, len(d), [base + i for i in range(m)], [base + i + 1 for i in range(m)]
