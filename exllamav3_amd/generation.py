"""
Token generation on top of the decode pipelines of llama_path.SyntheticEXL3Llama (which inherits GenerationMixin): embedding table, device-side sampler + token
feed, prompt ingestion through the prefill route, generate() and its speculative variant.  The host side of the loop -- stop arguments, the one graph capture,
the replay driver, the cut rules for the new tokens -- is written once as plain functions that need no GPU (tests/test_generation_host.py).
"""
from __future__ import annotations
from contextlib import contextmanager
import os
from types import SimpleNamespace
import torch
from . import ext, sampling


def parse_stop(stop_token_ids, stop_check_every, always_poll: bool = False):
    """generate()'s stop arguments -> (stop ids as a list | None, replays between two reads of the live word | None = no polling).  1 to sampling.MAX_STOP_IDS
    ids; the interval defaults to 16.  always_poll (the speculative path: the loop also leaves when the budget is used up): polling with or without ids;
    otherwise an interval without ids is an error."""
    stop = None
    if stop_token_ids is not None:
        stop = [int(t) for t in stop_token_ids]
        if not (1 <= len(stop) <= sampling.MAX_STOP_IDS):
            raise ValueError("generate: 1 to 64 stop token ids")
    elif not always_poll:
        if stop_check_every is not None:
            raise ValueError("generate: stop_check_every needs stop_token_ids")
        return None, None
    every = 16 if stop_check_every is None else int(stop_check_every)
    if every < 1:
        raise ValueError("generate: stop_check_every must be at least 1")
    return stop, every


def capture_once(body, device) -> torch.cuda.CUDAGraph:
    """body() -- kernel launches only -- captured as one graph on a side stream."""
    st = torch.cuda.Stream(device=device)
    st.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(st):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            body()
    torch.cuda.current_stream(device).wait_stream(st)
    return graph


def replay_loop(replay, n: int, every: int | None, read_live):
    """replay() up to n times with nothing in between -- no synchronisation, no host read -- except, with `every`, one read_live() behind every `every`-th replay
    that is not the last; leaves when that returns 0.  Returns (replays, polls, left_after): left_after = the replay count of an early exit, else None."""
    polls = 0
    for i in range(n):
        replay()
        if every is not None and (i + 1) % every == 0 and i + 1 < n:
            polls += 1
            if read_live() == 0:
                return i + 1, polls, i + 1
    return n, polls, None


def finish_tokens(new, one: bool, stop=None, eos_token_id: int | None = None) -> torch.Tensor:
    """The host-side cut rules for the new tokens [bsz, n]: one sequence is cut behind its first stop token (kept), a batch is filled with stop[0] behind each
    row's first stop token; then the same for eos_token_id with itself as the fill.  Returns int64 [n'] for one sequence, [bsz, n] for a batch."""
    def cut(new, ids, fill):
        for r in range(new.shape[0]):
            hit = torch.isin(new[r], torch.tensor(ids)).nonzero().flatten()
            if hit.numel():
                if one:
                    new = new[:, :int(hit[0]) + 1]
                else:
                    new[r, int(hit[0]) + 1:] = fill
        return new
    new = torch.as_tensor(new, dtype=torch.long)
    if stop is not None:
        new = cut(new, stop, stop[0])
    if eos_token_id is not None:
        new = cut(new, [eos_token_id], eos_token_id)
    return new[0] if one else new


class GenerationMixin:
    """The token generator of SyntheticEXL3Llama (llama_path.py), which supplies the state (alloc_state's buffers), the decode steps and _prefill_qkv_attend."""
    @contextmanager
    def _generating(self):
        """What both loops run inside: the decode attention on (restored on the way out) and a fresh gen_stats."""
        att_before = self.with_attention
        self.with_attention = True
        try:
            self.gen_stats = {"graph_captures": 0, "graph_replays": 0, "host_reads": 0}
            yield self.gen_stats
        finally:
            self.with_attention = att_before

    def _capture_and_replay(self, body, n: int, every: int | None, live: torch.Tensor):
        """body captured once, replayed up to n times (replay_loop; the poll reads the 4-byte `live` word, which synchronises); counts into gen_stats.  Returns
        the replay count at which the loop was left early, else None."""
        graph = capture_once(body, self.device)
        self.gen_stats["graph_captures"] = 1
        self.gen_stats["graph_replays"], polls, left_after = replay_loop(graph.replay, n, every, lambda: int(live.cpu()))
        self.gen_stats["host_reads"] += polls
        return left_after

    # ---- embedding table, device-side sampler + token feed, generate() ------------------------------------------------------------
    #: seed of a synthetic model's embedding table (its own generator: neither the host PCG64 stream of host_seed nor the device generator of `seed` is advanced)
    embed_seed = 20261016

    def embed_table(self) -> torch.Tensor:
        """fp16 [vocab, hidden] embedding table, created on the first call: `model.embed_tokens.weight` of the checkpoint the model was loaded from, else
        seeded random rows of unit RMS (what alloc_state feeds the step).  save_checkpoint writes it when present."""
        if getattr(self, "_embed", None) is None:
            s = self.shape
            src = getattr(self, "_embed_source", None)
            if src is not None:
                if not src.has_tensor("model.embed_tokens.weight"):
                    raise NotImplementedError("the checkpoint has no model.embed_tokens.weight (tied embeddings are not on this path)")
                self._embed = src.get_tensor("model.embed_tokens.weight", self.device).half().contiguous()
            else:
                g = torch.Generator(device=self.device)
                g.manual_seed(self.embed_seed)
                self._embed = torch.randn((s.vocab, s.hidden), device=self.device, generator=g, dtype=torch.float).half()
            assert self._embed.shape[0] >= s.vocab and self._embed.shape[1] == s.hidden, "embedding table does not match the model's shape"
        return self._embed

    def alloc_gen_state(self, bsz: int, max_new: int, prompt):
        """alloc_state for a generation from an EMPTY cache: positions start at 0 and everything alloc_state sizes by `pos` (the split-attention workspace, the
        max_len argument of the launch-per-op attention) is sized by max_ctx.  prompt: token ids [bsz, P] (P >= 1, one length for all rows).  The first prompt
        token reaches the step's input row through the same entry as every later token (sampling.gen_feed, step word -1 -> 0)."""
        dev = self.device
        prompt = torch.as_tensor(prompt, dtype=torch.long)
        assert prompt.dim() == 2 and prompt.shape[0] == bsz and prompt.shape[1] >= 1, "prompt must be [bsz, P] with P >= 1"
        assert 1 <= bsz <= sampling.MAX_ROWS, "the sampler takes 1..16 rows"
        P = prompt.shape[1]
        assert max_new >= 0 and P + max_new <= self.max_ctx, "prompt + new tokens exceed max_ctx"
        assert int(prompt.min()) >= 0 and int(prompt.max()) < self.shape.vocab, "prompt token outside the vocabulary"
        embed = self.embed_table()
        self._alloc_state(bsz, self.max_ctx - 1, torch.zeros((bsz, self.shape.hidden), dtype=torch.half, device=dev))
        total = max(P - 1 + max_new, 1)
        self.gen = SimpleNamespace(
            P=P, total=P - 1 + max_new, embed=embed, forced=prompt.to(torch.int32).to(dev).contiguous(),
            tokens_out=torch.empty((bsz, total), dtype=torch.int32, device=dev), sampled=torch.empty((bsz,), dtype=torch.int32, device=dev),
            invalid=torch.empty((bsz,), dtype=torch.int32, device=dev), step=torch.empty((1,), dtype=torch.int64, device=dev),
            ws=sampling.workspace(bsz, dev),
            # stop tokens (exl3_gen_feed_stop) and logit processors (exl3_logit_process): used only when generate() is given them
            done=torch.zeros((bsz,), dtype=torch.int32, device=dev), live=torch.full((1,), bsz, dtype=torch.int32, device=dev), stop_ids=None, proc_logits=None)
        self._gen_prime()
        return self.gen

    def _gen_prime(self):
        """(Re)starts the generation state: counters one step before the first token, then the priming feed (forced[:, 0] -> x0, counters and step word + 1)."""
        gs = self.gen
        self.positions.fill_(-1); self.cache_seqlens.fill_(-1); self.attn_lens.fill_(0)
        gs.step.fill_(-1); gs.invalid.zero_(); gs.tokens_out.fill_(-1); gs.sampled.fill_(-1)
        gs.done.zero_(); gs.live.fill_(self.x0.shape[0])
        sampling.gen_feed(None, gs.forced, gs.embed, self.x0, None, self.positions, self.cache_seqlens, self.attn_lens, gs.invalid, gs.step, vocab=self.shape.vocab)

    def gen_step(self, ka, processors=None, stop: bool = False):
        """The loop body of generate(): decode step, (logit processors,) sampler, token feed -- kernel launches only (graph-capturable).  processors: the sampler
        reads a second buffer that exl3_logit_process fills from the step's logits and the tokens fed so far (forced[:, 0], then tokens_out[:, :step word]).
        stop: the feed is exl3_gen_feed_stop over gs.stop_ids / gs.done / gs.live."""
        gs = self.gen
        logits = self.decode_step_auto()
        if processors is not None:
            logits = sampling.process_logits(logits, processors, gs.forced[:, 0:1], gs.tokens_out, step=gs.step, size=self.shape.vocab, out=gs.proc_logits)
        sampling.sample(logits, ka, gs.step, size=self.shape.vocab, out=gs.sampled, ws=gs.ws)
        if stop:
            sampling.gen_feed(gs.sampled, gs.forced, gs.embed, self.x0, gs.tokens_out, self.positions, self.cache_seqlens, self.attn_lens, gs.invalid, gs.step,
                              vocab=self.shape.vocab, stop_ids=gs.stop_ids, done=gs.done, pad_token=gs.pad_token, live=gs.live)
        else:
            sampling.gen_feed(gs.sampled, gs.forced, gs.embed, self.x0, gs.tokens_out, self.positions, self.cache_seqlens, self.attn_lens, gs.invalid, gs.step,
                              vocab=self.shape.vocab)

    #: tokens per row of one ingestion chunk of generate(prompt_mode="prefill").  Measured (tools/bench_generate.py, section prompt; 8191 prompt tokens, ingest_prompt
    #: alone): 512 / 1024 / 2048 / 4096 -> 29.5k / 42.8k / 59.5k / 72.1k tok/s on Llama-3.1-8B, 104k / 185k / 271k / 353k on Llama-3.2-1B: the largest wins (the
    #: weights are reconstructed once per chunk).  EXL3_HIP_GEN_PREFILL_CHUNK overrides it for A/B runs.
    gen_prefill_chunk = int(os.environ.get("EXL3_HIP_GEN_PREFILL_CHUNK", "4096"))

    def ingest_prompt(self, n_tokens: int, chunk: int | None = None, return_rows: bool = False, *, ids: torch.Tensor | None = None,
                      block_table: torch.Tensor | None = None, cache_seqlens: torch.Tensor | None = None, attn_lens: torch.Tensor | None = None,
                      invalid: torch.Tensor | None = None):
        """Prompt tokens 0 .. n_tokens - 1 of every row of the generation state (alloc_gen_state: gs.forced) through the PREFILL route into the generation's own
        cache (self.kcache / self.vcache per layer, through the state's block_table), at most `chunk` tokens per row at a time (default gen_prefill_chunk).  A chunk
        at offset p0 with T tokens: rows from exl3_embed_rows, then per layer RMSNorm -> q|k|v -> RoPE at p0 .. p0 + T - 1 -> quantised append behind
        cache_seqlens = p0 -> dequant_cache_paged into ONE fp16 expansion buffer shared by all layers (bsz * max_ctx rows) -> causal attention with lengths
        p0 + T -> o_proj (+ residual) -> norm -> gate|up -> down (+ residual).  Any T >= 1 works (LinearEXL3 routes by row count).  In the last chunk the last layer
        stops behind its cache append: nothing downstream of it is consumed (no final norm, no lm_head).  return_rows (tests): every layer runs to its end and the
        residual stream behind the last layer comes back as fp16 [bsz, n_tokens, hidden].
        Leaves positions = cache_seqlens = n_tokens and attn_lens = n_tokens + 1 (what a decode step of token n_tokens expects).  Returns the chunk count (or the rows).
        ids / block_table / cache_seqlens / attn_lens / invalid (all five together; the speculative path: one sequence inside a state of m aliased rows): the int32
        id matrix [rows, >= n_tokens], the block-table rows and the per-row counters to work on instead of the generation state's; the two counters are left at
        n_tokens / n_tokens + 1 and self.positions is not touched."""
        if self.tp > 1:
            raise NotImplementedError("ingest_prompt: tensor-parallel generation is not built")
        s, hd, dev = self.shape, self.shape.head_dim, self.device
        if hd not in (64, 128):
            raise NotImplementedError("ingest_prompt: the prefill attention takes head_dim 64 or 128")
        own = ids is None
        if own:
            if not (block_table is None and cache_seqlens is None and attn_lens is None and invalid is None):
                raise ValueError("ingest_prompt: ids, block_table, cache_seqlens, attn_lens and invalid go together")
            gs, bsz = self.gen, self._state_bsz
            ids, block_table, cache_seqlens, attn_lens, invalid = gs.forced, self.block_table, self.cache_seqlens, self.attn_lens, gs.invalid
        else:
            if block_table is None or cache_seqlens is None or attn_lens is None or invalid is None:
                raise ValueError("ingest_prompt: ids, block_table, cache_seqlens, attn_lens and invalid go together")
            bsz = ids.shape[0]
            if not (block_table.shape[0] == bsz and cache_seqlens.numel() == bsz and attn_lens.numel() == bsz and invalid.numel() >= bsz):
                raise ValueError("ingest_prompt: one block-table row and one counter per row of ids")
        n = int(n_tokens)
        chunk = int(self.gen_prefill_chunk if chunk is None else chunk)
        if chunk < 1:
            raise ValueError("ingest_prompt: chunk must be at least 1")
        if not (0 <= n <= ids.shape[1] and n <= self.max_ctx):
            raise ValueError("ingest_prompt: n_tokens outside the prompt")
        kv_dim = self.hkv * hd
        n_pages = self.kcache[0][0].shape[0]
        if getattr(self, "_ing_pages", None) is None or self._ing_pages[0].shape != (n_pages, self.page, kv_dim):
            self._ing_pages = [torch.zeros((n_pages, self.page, kv_dim), dtype=torch.half, device=dev) for _ in range(2)]
        kd, vd = self._ing_pages
        out, chunks = [], 0
        for p0 in range(0, n, chunk):
            T = min(chunk, n - p0)
            cache_seqlens.fill_(p0)
            attn_lens.fill_(p0 + T)
            x = sampling.embed_rows(ids, p0, T, self.embed_table(), invalid, vocab=s.vocab)
            xn = torch.empty_like(x)
            ao = torch.empty((bsz * T, self.hq * hd), dtype=torch.half, device=dev)
            for li, L in enumerate(self.layers):
                ext.rms_norm(x, L["norm1"], xn, self.eps)
                last = p0 + T == n and li == self.n_layers - 1 and not return_rows
                q = self._prefill_qkv_attend(L, xn, bsz, T, p0, self.kcache[li], self.vcache[li], cache_seqlens, block_table,
                                             None if last else (kd, vd, attn_lens, ao))
                if last:
                    break
                L["o"].forward_add_residual(q, x)
                ext.rms_norm(x, L["norm2"], xn, self.eps)
                a = type(L["gate"]).forward_gate_up_silu(L["gate"], L["up"], xn)
                L["down"].forward_add_residual(a, x)
            chunks += 1
            if return_rows:
                out.append(x.view(bsz, T, s.hidden))
        if own:
            self.positions.fill_(n)
        cache_seqlens.fill_(n); attn_lens.fill_(n + 1)
        return torch.cat(out, dim=1) if return_rows else chunks

    def _gen_prime_prefilled(self, chunk: int | None = None) -> int:
        """_gen_prime for generate(prompt_mode="prefill"): prompt tokens 0 .. P - 2 go through ingest_prompt, then the state is set to what P - 2 replays of the
        loop leave (step word = positions = cache_seqlens = P - 2, attn_lens = P - 1, tokens_out[:, :P - 2] = prompt[:, 1:P - 1]) and ONE feed without sampled
        tokens does the rest as it does in the loop: forced[:, P - 1] -> x0 and tokens_out[:, P - 2], every counter + 1.  Integer for integer the state behind
        P - 1 replays, so the logit processors see the same history and the sampler the same step words.  Returns the chunk count."""
        gs, P = self.gen, self.gen.P
        assert P >= 2, "nothing to ingest"
        self._gen_prime()
        chunks = self.ingest_prompt(P - 1, chunk)
        self.positions.fill_(P - 2); self.cache_seqlens.fill_(P - 2); self.attn_lens.fill_(P - 1)
        gs.step.fill_(P - 2)
        gs.tokens_out[:, :P - 2] = gs.forced[:, 1:P - 1]
        sampling.gen_feed(None, gs.forced, gs.embed, self.x0, gs.tokens_out, self.positions, self.cache_seqlens, self.attn_lens, gs.invalid, gs.step, vocab=self.shape.vocab)
        return chunks

    def generate(self, prompt_ids, max_new_tokens: int, settings=None, eos_token_id: int | None = None, processors=None, stop_token_ids=None,
                 stop_check_every: int | None = None, prompt_mode: str = "decode", prefill_chunk: int | None = None, speculative=None) -> torch.Tensor:
        """Generates max_new_tokens tokens behind prompt_ids ([P] or [bsz, P]) from an empty cache, with the decode attention on.  The loop body (decode_step_auto +
        sampler + token feed) is captured ONCE as a graph and replayed P - 1 + max_new_tokens times without a synchronisation or a host read in between (the
        prompt goes through the same step token by token as forced tokens: prompt_mode "decode", the default); one read at the end.
        prompt_mode "prefill": prompt tokens 0 .. P - 2 go through the prefill route instead (ingest_prompt, chunks of prefill_chunk tokens per row, default
        gen_prefill_chunk), one feed hands the state over (_gen_prime_prefilled) and the captured body is replayed max_new_tokens times; gen_stats gains
        prefill_tokens (bsz * (P - 1)) and prefill_chunks on this path only.  With P == 1 there is nothing to ingest: decode mode.  One
        uncaptured step runs first (decode_step_persistent checks a new plan's first run for time-outs only outside capture); the state is reset after it.
        settings: sampling.SamplerSettings (None = greedy).  Returns int64 [n] / [bsz, n]: the new tokens, for one sequence trimmed behind the first
        eos_token_id (kept), for a batch filled with eos_token_id behind it.  Raises if a row went invalid (NaN logits: a timed-out persistent step).
        processors: sampling.LogitProcessors -- one more launch per token (exl3_logit_process) between the step and the sampler, still no host read.
        stop_token_ids (<= 64 ids): the feed marks a row done at its first SAMPLED stop token (a stop id inside the prompt does not count); after every
        stop_check_every replays (default 16) the host reads the 4-byte live word and leaves the loop when no row is live.  The result follows the EOS rules: one
        sequence is cut behind its first stop token (kept), a batch is filled with the first stop id behind it.  gen_stats counts the reads of the live word in
        host_reads and gains stopped_after (the replay count at which the loop was left early, else None) on this path only.
        speculative: sampling.SpeculativeSettings -- one sequence, several tokens per weight pass where the drafts hold (_generate_speculative); the tokens are
        those of the same loop without drafts; the prompt always takes the prefill route (prompt_mode is not read), stop_check_every applies with or without
        stop ids (the loop leaves when the budget is used up), processors and batches are refused.  None (the default): everything above, unchanged."""
        if prompt_mode not in ("decode", "prefill"):
            raise ValueError('generate: prompt_mode is "decode" or "prefill"')
        if self.tp > 1:
            raise NotImplementedError("generate: tensor-parallel sampling (the vocabulary gather) is not built")
        if self.shape.head_dim not in (64, 128):
            raise NotImplementedError("generate: the decode attention takes head_dim 64 or 128")
        if speculative is not None:
            return self._generate_speculative(prompt_ids, max_new_tokens, settings, eos_token_id, processors, stop_token_ids, stop_check_every, prefill_chunk, speculative)
        prompt = torch.as_tensor(prompt_ids, dtype=torch.long)
        one = prompt.dim() == 1
        if one:
            prompt = prompt.unsqueeze(0)
        bsz, P = prompt.shape
        ka = (settings or sampling.SamplerSettings(temperature=0.0)).kernel_args()
        if processors is not None and processors.is_noop:
            processors = None
        stop, every = parse_stop(stop_token_ids, stop_check_every)
        with self._generating() as stats:
            gs = self.alloc_gen_state(bsz, max_new_tokens, prompt)
            if stop is not None:
                stats["stopped_after"] = None
                gs.stop_ids = torch.tensor(stop, dtype=torch.int32, device=self.device)
                gs.pad_token = stop[0]
            if processors is not None:
                gs.proc_logits = torch.empty_like(self.logits)
            prefill = prompt_mode == "prefill" and P > 1
            replays = max_new_tokens if prefill else gs.total
            if replays > 0:
                def body(): self.gen_step(ka, processors, stop is not None)
                body()                                             # uncaptured: plan creation, the persistent step's first-run check (may fall back, loudly)
                if prefill:
                    stats["prefill_chunks"] = self._gen_prime_prefilled(prefill_chunk)
                    stats["prefill_tokens"] = bsz * (P - 1)
                else:
                    self._gen_prime()
                left_after = self._capture_and_replay(body, replays, every, gs.live)
                if stop is not None:
                    stats["stopped_after"] = left_after
            host = torch.cat([gs.tokens_out, gs.invalid.view(bsz, 1)], dim=1).cpu()           # the one read (synchronises)
            stats["host_reads"] += 1
        toks, invalid = host[:, :gs.total].long(), host[:, -1]
        if bool(invalid.any()):
            ps = getattr(self, "_pstep", None)
            if ps is not None and ps.tp is None and ps.error():
                self._retire_timed_out_pstep()
            raise RuntimeError(f"generate: rows {[int(i) for i in invalid.nonzero().flatten()]} produced an invalid token (NaN / Inf logits)")
        return finish_tokens(toks[:, P - 1:], one, stop, eos_token_id)

    # ---- speculative decoding: one sequence as m aliased rows, accept / draft / feed on the device (csrc/exl3_spec.hip) ------------------------------------
    #: the launches behind the sampler of a verify step: True = exl3_spec_round (accept + draft + feed in one launch), False = exl3_spec_accept then
    #: exl3_spec_draft_ngram (tools/bench_generate.py, section speculative, measures both)
    spec_fold = os.environ.get("EXL3_HIP_SPEC_FOLD", "1") != "0"

    def alloc_spec_state(self, k: int, max_new: int, prompt, settings=None):
        """The state of a speculative generation of ONE sequence with k drafts per verify step: _alloc_state's buffers for m = k + 1 rows, but cache pages for one
        sequence and a block table whose m rows all name them (row i of a verify step is position base + i of that sequence); every workspace sized by
        max_ctx as in alloc_gen_state.  prompt: token ids [P], P >= 1.  Requires P + max_new + k <= max_ctx: the padding rows of the last round append their
        K / V beyond the token budget.  settings: sampling.SpeculativeSettings (match lengths, script).  Primed: hist[:P] = prompt, base = P - 1, the first
        round's inputs written by the drafter (the cache is still empty: ingest the prompt's first P - 1 tokens before the first spec_step)."""
        dev = self.device
        settings = settings or sampling.SpeculativeSettings()                  # (only the match lengths and the script are read here: k = 0 is a legal state)
        k = int(k)
        m = k + 1
        if not (1 <= m <= sampling.MAX_ROWS):
            raise ValueError("alloc_spec_state: k must be in [0, 15]")
        prompt = torch.as_tensor(prompt, dtype=torch.long).flatten()
        P = prompt.numel()
        if P < 1 or max_new < 0:
            raise ValueError("alloc_spec_state: the prompt holds at least one token, max_new is not negative")
        if P + max_new + k > self.max_ctx:
            raise ValueError(f"alloc_spec_state: prompt ({P}) + new tokens ({max_new}) + drafts ({k}) exceed max_ctx ({self.max_ctx})")
        if int(prompt.min()) < 0 or int(prompt.max()) >= self.shape.vocab:
            raise ValueError("alloc_spec_state: prompt token outside the vocabulary")
        embed = self.embed_table()
        self._alloc_state(m, self.max_ctx - 1, torch.zeros((m, self.shape.hidden), dtype=torch.half, device=dev), one_sequence=True)
        script = None
        if settings.script is not None:
            sc = torch.as_tensor(settings.script, dtype=torch.long).flatten()[:self.max_ctx]
            script = torch.full((self.max_ctx,), -1, dtype=torch.int32)
            script[:sc.numel()] = sc.to(torch.int32)
            script = script.to(dev)
        i32 = torch.int32
        self.spec = SimpleNamespace(
            k=k, m=m, P=P, max_new=int(max_new), embed=embed, prompt=prompt.to(i32).to(dev), script=script, stop_ids=None,
            match_min=int(settings.ngram_match_min), match_max=int(settings.ngram_match_max),
            hist=torch.empty((self.max_ctx,), dtype=i32, device=dev), state=torch.empty((sampling.SPEC_STATE_WORDS,), dtype=i32, device=dev),
            state0=torch.tensor([P - 1, 0, 1 if max_new > 0 else 0, 0, 0, 0, 0, 0, 0], dtype=i32, device=dev),
            round=torch.empty((1,), dtype=torch.int64, device=dev), in_tokens=torch.empty((m,), dtype=i32, device=dev),
            sampled=torch.empty((m,), dtype=i32, device=dev), tokens_out=torch.empty((max(int(max_new), 1),), dtype=i32, device=dev),
            ing_invalid=torch.zeros((1,), dtype=i32, device=dev), ws=sampling.workspace(m, dev))
        self.spec.live = self.spec.state[sampling.SPEC_LIVE:sampling.SPEC_LIVE + 1]            # the 4-byte word the host polls
        self._spec_prime()
        return self.spec

    def _spec_prime(self):
        """(Re)starts the speculative state: history = the prompt, base = P - 1, nothing produced, round word 0, then the drafter's launch writes the inputs of
        the first verify step.  The cache is left as it is (positions below P - 1 hold the ingested prompt; everything from P - 1 on is rewritten)."""
        sp = self.spec
        sp.hist.fill_(-1); sp.hist[:sp.P] = sp.prompt
        sp.state.copy_(sp.state0); sp.round.zero_(); sp.tokens_out.fill_(-1); sp.sampled.fill_(-1)
        sampling.spec_draft(sp.hist, sp.state, sp.in_tokens, sp.embed, self.x0, self.positions, self.cache_seqlens, self.attn_lens, sp.k, sp.max_new,
                            sp.match_min, sp.match_max, script=sp.script, vocab=self.shape.vocab)

    def spec_step(self, ka, stop: bool = False):
        """The loop body of speculative generation -- kernel launches only (graph-capturable): the verify step over the m aliased rows, the sampler over the m
        logits rows with step word = round, then accept / draft / feed (one launch, or two with spec_fold off).
        The verify step is decode_step_fused for EVERY m, m = 2 included, not decode_step_auto: row i attends over what rows < i append in the same step, so
        all m appends must be complete before any row attends.  decode_step_fused appends every row in glue_qkv and attends in a later launch.
        decode_step_fx (what decode_step_auto picks at 2-4 rows) appends inside the context-split attention launch itself, where the workgroup that holds a
        row's new token writes it while other rows' workgroups already read; the persistent step takes one row only."""
        sp = self.spec
        logits = self.decode_step_fused()
        sampling.sample(logits, ka, sp.round, size=self.shape.vocab, out=sp.sampled, ws=sp.ws)
        stop_ids = sp.stop_ids if stop else None
        if self.spec_fold:
            sampling.spec_round(sp.sampled, sp.in_tokens, sp.state, sp.round, sp.hist, sp.tokens_out, sp.embed, self.x0, self.positions, self.cache_seqlens,
                                self.attn_lens, sp.k, sp.match_min, sp.match_max, script=sp.script, stop_ids=stop_ids, vocab=self.shape.vocab, max_new=sp.max_new)
        else:
            sampling.spec_accept(sp.sampled, sp.in_tokens, sp.state, sp.round, sp.hist, sp.tokens_out, self.shape.vocab, stop_ids=stop_ids, max_new=sp.max_new)
            sampling.spec_draft(sp.hist, sp.state, sp.in_tokens, sp.embed, self.x0, self.positions, self.cache_seqlens, self.attn_lens, sp.k, sp.max_new,
                                sp.match_min, sp.match_max, script=sp.script, vocab=self.shape.vocab)

    def _spec_ingest(self, chunk: int | None = None) -> int:
        """Prompt tokens 0 .. P - 2 of the speculative state through the prefill route into the one sequence's cache (ingest_prompt over row 0's block-table row
        and counters; the prime behind it rewrites the counters).  Returns the chunk count."""
        sp = self.spec
        return self.ingest_prompt(sp.P - 1, chunk, ids=sp.hist.view(1, -1), block_table=self.block_table[:1], cache_seqlens=self.cache_seqlens[:1],
                                  attn_lens=self.attn_lens[:1], invalid=sp.ing_invalid)

    def _generate_speculative(self, prompt_ids, max_new_tokens, settings, eos_token_id, processors, stop_token_ids, stop_check_every, prefill_chunk, spec):
        """generate(..., speculative=spec): one sequence; every verify step (spec_step) runs num_draft_tokens + 1 rows and commits the drafts that equal the
        target's own tokens plus one.  Prompt tokens 0 .. P - 2 go through the prefill route (P == 1: nothing to ingest), one uncaptured round runs, the state
        is reset, the body is captured ONCE and replayed at most max_new_tokens times; after every stop_check_every replays (default 16) the host reads the
        4-byte live word and leaves when it is 0 (budget used up, stop token, invalid); one read at the end.  gen_stats gains spec_rounds, spec_drafted and
        spec_accepted (live rounds, drafts fed, drafts accepted: spec_accepted + spec_rounds = tokens produced).
        Sampled modes: the draft is deterministic and row i's token is drawn from the target's distribution with noise that depends on (row, round) only; a
        draft is accepted iff it equals that token, else the token itself is emitted -- the output distribution is exactly the target's."""
        if not isinstance(spec, sampling.SpeculativeSettings):
            raise TypeError("generate: speculative must be a sampling.SpeculativeSettings")
        if processors is not None:
            raise NotImplementedError("generate: logit processors under speculation are not built (the penalty windows of rows >= 1 would have to include the drafts)")
        prompt = torch.as_tensor(prompt_ids, dtype=torch.long)
        one = prompt.dim() == 1
        if not one:
            if not (prompt.dim() == 2 and prompt.shape[0] == 1):
                raise NotImplementedError("generate: speculative decoding of a batch of sequences is not built")
            prompt = prompt[0]
        P, max_new, k = prompt.numel(), int(max_new_tokens), int(spec.num_draft_tokens)
        ka = (settings or sampling.SamplerSettings(temperature=0.0)).kernel_args()
        stop, every = parse_stop(stop_token_ids, stop_check_every, always_poll=True)
        with self._generating() as stats:
            sp = self.alloc_spec_state(k, max_new, prompt, spec)               # (refuses an empty prompt and a budget beyond max_ctx)
            if stop is not None:
                stats["stopped_after"] = None
                sp.stop_ids = torch.tensor(stop, dtype=torch.int32, device=self.device)
            if max_new > 0:
                def body(): self.spec_step(ka, stop is not None)
                if P > 1:
                    stats["prefill_chunks"] = self._spec_ingest(prefill_chunk)
                    stats["prefill_tokens"] = P - 1
                    self._spec_prime()
                body()                                             # uncaptured: plan creation
                self._spec_prime()
                left_after = self._capture_and_replay(body, max_new, every, sp.live)
                if stop is not None:
                    stats["stopped_after"] = left_after
            host = torch.cat([sp.tokens_out, sp.state, sp.ing_invalid]).cpu()                  # the one read (synchronises)
            stats["host_reads"] += 1
        n_out = sp.tokens_out.numel()
        state = host[n_out:n_out + sampling.SPEC_STATE_WORDS].tolist()
        stats.update(spec_rounds=state[sampling.SPEC_ROUNDS], spec_drafted=state[sampling.SPEC_DRAFTED], spec_accepted=state[sampling.SPEC_ACCEPTED])
        if state[sampling.SPEC_INVALID] or int(host[-1]):
            raise RuntimeError("generate: the sequence produced an invalid token (NaN / Inf logits)")
        if stop is not None and stats["stopped_after"] is None and state[sampling.SPEC_DONE]:
            stats["stopped_after"] = stats["graph_replays"]
        new = finish_tokens(host[:state[sampling.SPEC_PRODUCED]].view(1, -1), True, None, eos_token_id)     # (the stop cut is the device's: SPEC_PRODUCED)
        return new if one else new.unsqueeze(0)

