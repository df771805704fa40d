// Speculative decoding between two verify steps: accept / roll back (exl3_spec_accept), draft + feed (exl3_spec_draft_ngram), or both in one launch
// (exl3_spec_round).  gfx950 only.
//
// A verify step for k drafts is a decode step over m = k + 1 rows of ONE sequence (llama_path.py: spec_step): row 0 carries the last committed token, row i a
// draft, row i's logits are the target's distribution for position base + i + 1.  The sampler draws one token per row; the accept launch commits the run of drafts
// that equal the target's own choices plus the one token behind it, and the draft launch proposes the next drafts and writes the step's next inputs.  The
// reference runs this logic on the host (generator/job.py); here it sits inside the replayed graph, so everything is a function of device words.
//
// One workgroup per launch (m <= 16 rows; the n-gram scan is max_ctx positions x <= 16 compares): no workgroup ever waits for another, nothing is allocated.
//   state (int32 words): SPEC_BASE      position of the last committed token (hist[0 .. base] is committed)
//                        SPEC_PRODUCED  new tokens emitted so far        SPEC_LIVE  1 while another round can emit a token
//                        SPEC_DONE      a stop id was emitted (sticky)   SPEC_INVALID  a consumed sample lay outside the vocabulary (sticky)
//                        SPEC_NDRAFT    drafts among in_tokens[1 ..]     SPEC_ROUNDS / SPEC_DRAFTED / SPEC_ACCEPTED  counters over live rounds
#include "exl3_api_internal.h"
#include "exl3_common.cuh"

#define SPEC_MAX_ROWS   16
#define SPEC_MAX_MATCH  16
#define SPEC_MAX_STOP   64
#define SPEC_THREADS    1024
enum { SPEC_BASE = 0, SPEC_PRODUCED, SPEC_LIVE, SPEC_DONE, SPEC_INVALID, SPEC_NDRAFT, SPEC_ROUNDS, SPEC_DRAFTED, SPEC_ACCEPTED, SPEC_STATE_WORDS };

struct SpecAcceptArgs
{
    const int32_t* sampled; const int32_t* in_tokens; int m; int vocab; int32_t* state; long long* round; int32_t* hist; int max_ctx;
    int32_t* tokens_out; int max_new; const int32_t* stop_ids; int n_stop;
};
struct SpecDraftArgs
{
    const int32_t* hist; int max_ctx; const int32_t* script; int k; int match_min; int match_max; int m; int32_t* state; int32_t* in_tokens;
    const half_t* embed; int vocab; int hidden; half_t* x0; int32_t* positions; int32_t* cache_seqlens; int32_t* attn_lens;
};

__device__ __forceinline__ bool spec_frozen(const int32_t* st, int max_new) { return st[SPEC_DONE] || st[SPEC_INVALID] || st[SPEC_PRODUCED] >= max_new; }

// The only place state advances.  One thread: at most 16 rows x 64 stop ids.
__device__ void spec_accept_thread0(const SpecAcceptArgs& a)
{
    int32_t* st = a.state;
    *a.round += 1;
    if (spec_frozen(st, a.max_new)) { st[SPEC_LIVE] = 0; return; }
    const int base = st[SPEC_BASE], produced = st[SPEC_PRODUCED];
    if (base < 0 || produced < 0) { st[SPEC_INVALID] = 1; st[SPEC_LIVE] = 0; return; }                     // (a state nobody initialised: nothing is indexed by it)
    int nd = st[SPEC_NDRAFT];
    nd = nd < 0 ? 0 : (nd > a.m - 1 ? a.m - 1 : nd);
    int n = 0;
    while (n < nd && a.in_tokens[n + 1] == a.sampled[n]) ++n;
    if (produced + n + 1 > a.max_new) n = a.max_new - produced - 1;
    int emitted = 0;
    for (int i = 0; i <= n; ++i)
    {
        const int tok = a.sampled[i];
        if (tok < 0 || tok >= a.vocab || base + 1 + i >= a.max_ctx) { st[SPEC_INVALID] = 1; break; }       // sticky: never reaches hist, so never indexes the table
        a.hist[base + 1 + i] = tok;
        a.tokens_out[produced + i] = tok;
        ++emitted;
        bool stop = false;
        for (int s = 0; s < a.n_stop; ++s) stop = stop || a.stop_ids[s] == tok;
        if (stop) { st[SPEC_DONE] = 1; break; }                                                            // the stop token is kept, nothing behind it
    }
    st[SPEC_BASE] = base + emitted;
    st[SPEC_PRODUCED] = produced + emitted;
    st[SPEC_ROUNDS] += 1;
    st[SPEC_DRAFTED] += nd;
    st[SPEC_ACCEPTED] += emitted > 0 ? emitted - 1 : 0;
    st[SPEC_LIVE] = !spec_frozen(st, a.max_new);
}

// Drafts for the committed history hist[0 .. base] and the inputs of the next verify step.  A frozen state changes nothing.
// hist is read through a plain pointer: in exl3_spec_round thread 0 wrote it in front of the barrier that precedes this call.
__device__ void spec_draft_feed(const SpecDraftArgs& a, int max_new)
{
    __shared__ unsigned long long best_s;
    __shared__ int tok_s[SPEC_MAX_ROWS];
    __shared__ int suffix_s[SPEC_MAX_MATCH];
    const int tid = threadIdx.x;
    const int32_t* st = a.state;
    if (spec_frozen(st, max_new)) return;                                       // uniform: every thread reads the same words
    const int base = st[SPEC_BASE];
    if (base < 0 || base + a.m - 1 >= a.max_ctx)                                // rows would append beyond the cache: refuse to feed
    {
        if (tid == 0) { a.state[SPEC_INVALID] = 1; a.state[SPEC_LIVE] = 0; }
        return;
    }
    const int L = base + 1;
    const int32_t* hist = a.hist;
    int e_best = 0, c = 0;
    if (a.script)
    {
        // scripted drafter: script[base + 1 ..] while the entries are valid ids
        if (tid == 0)
        {
            while (c < a.k && L + c < a.max_ctx && a.script[L + c] >= 0 && a.script[L + c] < a.vocab) ++c;
            for (int i = 0; i < c; ++i) tok_s[1 + i] = a.script[L + i];
            best_s = (unsigned long long) c;
        }
        __syncthreads();
        c = (int) best_s;
    }
    else
    {
        // n-gram drafter: per end position e the length of the common suffix of hist[0 .. e) and hist[0 .. L), capped at match_max; the maximum of (length, e)
        if (tid == 0) best_s = 0ull;
        if (tid < a.match_max) suffix_s[tid] = tid < L ? hist[L - 1 - tid] : -1;
        __syncthreads();
        unsigned long long best = 0ull;
        for (int e = 1 + tid; e <= L - 1; e += SPEC_THREADS)
        {
            const int cap = e < a.match_max ? e : a.match_max;
            int len = 0;
            while (len < cap && hist[e - 1 - len] == suffix_s[len]) ++len;
            if (len >= a.match_min)
            {
                const unsigned long long key = ((unsigned long long) len << 32) | (unsigned) e;
                best = key > best ? key : best;
            }
        }
        if (best) atomicMax(&best_s, best);
        __syncthreads();
        best = best_s;
        if (best)
        {
            e_best = (int) (best & 0xffffffffull);
            c = L - e_best < a.k ? L - e_best : a.k;
        }
        if (tid < c) tok_s[1 + tid] = hist[e_best + tid];
    }
    if (tid == 0) tok_s[0] = hist[base];
    __syncthreads();
    if (tid < a.m)
    {
        const int tok = tid <= c ? tok_s[tid] : tok_s[0];                       // padding rows repeat the committed token
        a.in_tokens[tid] = tok;
        a.positions[tid] = base + tid;
        a.cache_seqlens[tid] = base + tid;
        a.attn_lens[tid] = base + tid + 1;
    }
    if (tid == 0) a.state[SPEC_NDRAFT] = c;
    const int per_row = a.hidden / 8;
    for (int i = tid; i < a.m * per_row; i += SPEC_THREADS)
    {
        const int r = i / per_row, col = i - r * per_row;
        int tok = r <= c ? tok_s[r] : tok_s[0];
        tok = (tok >= 0 && tok < a.vocab) ? tok : 0;                            // (hist holds checked ids only; a foreign hist never indexes outside the table)
        ((uint4_t*) (a.x0 + (size_t) r * a.hidden))[col] = ((const uint4_t*) (a.embed + (size_t) tok * a.hidden))[col];
    }
}

__global__ __launch_bounds__(64)
void spec_accept_kernel(SpecAcceptArgs a)
{
    if (threadIdx.x == 0) spec_accept_thread0(a);
}

__global__ __launch_bounds__(SPEC_THREADS)
void spec_draft_kernel(SpecDraftArgs d, int max_new)
{
    spec_draft_feed(d, max_new);
}

// accept, then draft + feed, in one workgroup: the barrier orders thread 0's writes (state, hist) in front of every thread's reads
__global__ __launch_bounds__(SPEC_THREADS)
void spec_round_kernel(SpecAcceptArgs a, SpecDraftArgs d)
{
    if (threadIdx.x == 0) spec_accept_thread0(a);
    __threadfence_block();
    __syncthreads();
    spec_draft_feed(d, a.max_new);
}

static int spec_check_accept(const char* who, const int32_t* sampled, const int32_t* in_tokens, int m, int vocab, int32_t* state, int64_t* round, int32_t* hist,
                             int max_ctx, int32_t* tokens_out, int max_new, const int32_t* stop_ids, int n_stop)
{
    EXL3_CHECK_ARG(m >= 1 && m <= SPEC_MAX_ROWS, "%s: m must be in [1, 16]", who);
    EXL3_CHECK_ARG(sampled && in_tokens && state && round && hist && tokens_out, "%s: null pointer", who);
    EXL3_CHECK_ARG(vocab >= 1 && max_ctx >= 1 && max_new >= 0, "%s: vocab and max_ctx must be at least 1, max_new not negative", who);
    EXL3_CHECK_ARG(n_stop >= 0 && n_stop <= SPEC_MAX_STOP && (n_stop == 0 || stop_ids), "%s: at most 64 stop ids", who);
    return EXL3_OK;
}

static int spec_check_draft(const char* who, const int32_t* hist, int max_ctx, int k, int match_min, int match_max, int m, int32_t* state, int max_new,
                            int32_t* in_tokens, const void* embed, int vocab, int hidden, void* x0, int32_t* positions, int32_t* cache_seqlens, int32_t* attn_lens)
{
    EXL3_CHECK_ARG(m >= 1 && m <= SPEC_MAX_ROWS, "%s: m must be in [1, 16]", who);
    EXL3_CHECK_ARG(hist && state && in_tokens && embed && x0 && positions && cache_seqlens && attn_lens, "%s: null pointer", who);
    EXL3_CHECK_ARG(k >= 0 && k <= m - 1, "%s: k must be in [0, m - 1]", who);
    EXL3_CHECK_ARG(match_min >= 1 && match_min <= match_max, "%s: 1 <= match_min <= match_max", who);
    EXL3_CHECK_ARG(match_max <= SPEC_MAX_MATCH, "%s: match_max must be at most 16", who);
    EXL3_CHECK_ARG(vocab >= 1 && max_ctx >= 1 && max_new >= 0, "%s: vocab and max_ctx must be at least 1, max_new not negative", who);
    EXL3_CHECK_ARG(hidden >= 8 && hidden % 8 == 0, "%s: hidden must be a multiple of 8", who);
    EXL3_CHECK_ARG((((uintptr_t) embed | (uintptr_t) x0) & 15) == 0, "%s: embed / x0 must be 16-byte aligned", who);
    return EXL3_OK;
}

extern "C" int exl3_spec_accept(const int32_t* sampled, const int32_t* in_tokens, int m, int vocab, int32_t* state, int64_t* round, int32_t* hist, int max_ctx,
                                int32_t* tokens_out, int max_new, const int32_t* stop_ids, int n_stop, void* stream)
{
    if (int rc = spec_check_accept("exl3_spec_accept", sampled, in_tokens, m, vocab, state, round, hist, max_ctx, tokens_out, max_new, stop_ids, n_stop)) return rc;
    const SpecAcceptArgs a = {sampled, in_tokens, m, vocab, state, (long long*) round, hist, max_ctx, tokens_out, max_new, stop_ids, n_stop};
    spec_accept_kernel<<<1, 64, 0, (hipStream_t) stream>>>(a);
    return exl3_check_launch("spec_accept");
}

extern "C" int exl3_spec_draft_ngram(const int32_t* hist, int max_ctx, const int32_t* script, int k, int match_min, int match_max, int m, int32_t* state,
                                     int max_new, int32_t* in_tokens, const void* embed, int vocab, int hidden, void* x0, int32_t* positions,
                                     int32_t* cache_seqlens, int32_t* attn_lens, void* stream)
{
    if (int rc = spec_check_draft("exl3_spec_draft_ngram", hist, max_ctx, k, match_min, match_max, m, state, max_new, in_tokens, embed, vocab, hidden, x0, positions,
                                  cache_seqlens, attn_lens)) return rc;
    const SpecDraftArgs d = {hist, max_ctx, script, k, match_min, match_max, m, state, in_tokens, (const half_t*) embed, vocab, hidden, (half_t*) x0, positions,
                             cache_seqlens, attn_lens};
    spec_draft_kernel<<<1, SPEC_THREADS, 0, (hipStream_t) stream>>>(d, max_new);
    return exl3_check_launch("spec_draft_ngram");
}

extern "C" int exl3_spec_round(const int32_t* sampled, int32_t* in_tokens, int m, int vocab, int32_t* state, int64_t* round, int32_t* hist, int max_ctx,
                               int32_t* tokens_out, int max_new, const int32_t* stop_ids, int n_stop, const int32_t* script, int k, int match_min, int match_max,
                               const void* embed, int hidden, void* x0, int32_t* positions, int32_t* cache_seqlens, int32_t* attn_lens, void* stream)
{
    if (int rc = spec_check_accept("exl3_spec_round", sampled, in_tokens, m, vocab, state, round, hist, max_ctx, tokens_out, max_new, stop_ids, n_stop)) return rc;
    if (int rc = spec_check_draft("exl3_spec_round", hist, max_ctx, k, match_min, match_max, m, state, max_new, in_tokens, embed, vocab, hidden, x0, positions,
                                  cache_seqlens, attn_lens)) return rc;
    const SpecAcceptArgs a = {sampled, in_tokens, m, vocab, state, (long long*) round, hist, max_ctx, tokens_out, max_new, stop_ids, n_stop};
    const SpecDraftArgs d = {hist, max_ctx, script, k, match_min, match_max, m, state, in_tokens, (const half_t*) embed, vocab, hidden, (half_t*) x0, positions,
                             cache_seqlens, attn_lens};
    spec_round_kernel<<<1, SPEC_THREADS, 0, (hipStream_t) stream>>>(a, d);
    return exl3_check_launch("spec_round");
}
