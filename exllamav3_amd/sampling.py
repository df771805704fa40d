"""
Device-side sampling (csrc/exl3_sampler.hip, csrc/exl3_logit_process.hip; include/exl3_hip.h: exl3_sample / exl3_gen_feed / exl3_gen_feed_stop /
exl3_embed_rows / exl3_logit_process).

SamplerSettings collapses a (temperature, top-k, top-p, min-p) stack into the kernel's (mode, filters, ...) the way the reference collapses a sampler
stack into its fused sampler (generator/sampler/custom.py:267-343): greedy when nothing can change the top token, a Gumbel sample of softmax(l / T)
otherwise, restricted to one cutoff for min-p alone (mode 2) or for any combination with top-k / top-p (mode 3).

The noise is this library's own Philox4x32-10 stream keyed by (seed; column, row, step) -- NOT curand's sequence, so the reference's op names
(argmax_sample, gumbel_sample, fused_sampler, gumbel_noise_*) are deliberately absent from exllamav3_amd.ext.

LogitProcessors is what runs in front of the sampler: repetition and presence / frequency penalties over the tokens generated so far, a logit bias with banned
tokens, a packed token bitmask -- the deterministic steps of the reference's sampler stack (custom.py: SS_RepP, SS_PresFreqP, SS_LogitBias, SS_BanTokens and the
grammar filters' bitmask), collapsed the way the reference collapses them and applied by ONE launch (process_logits -> exl3_logit_process).
"""
from __future__ import annotations
import ctypes
import math
from dataclasses import dataclass
import torch
from . import _lib
from ._lib import check as _check

MODE_GREEDY, MODE_SAMPLE, MODE_SAMPLE_MINP, MODE_SAMPLE_FILTERS = 0, 1, 2, 3
F_TOPK, F_TOPP, F_MINP = 1, 2, 4
MAX_ROWS = 16


@dataclass(frozen=True)
class KernelArgs:
    mode: int
    filters: int
    top_k: int
    top_p: float
    inv_temp: float
    inv_temp_filter: float
    minp_log: float
    seed: int


@dataclass(frozen=True)
class SamplerSettings:
    """temperature 0 = greedy.  temperature_last: the filters see the untempered distribution and temperature applies to what they keep (the reference's
    default preset order); otherwise temperature comes first and the filters see softmax(l / T).  top_k 0, top_p 1 and min_p 0 switch their filter off."""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    temperature_last: bool = False
    seed: int = 0

    def kernel_args(self) -> KernelArgs:
        T, k, p, mp = float(self.temperature), int(self.top_k), float(self.top_p), float(self.min_p)
        if T < 0 or k < 0 or not (0.0 <= p <= 1.0) or not (0.0 <= mp <= 1.0):
            raise ValueError("SamplerSettings: temperature >= 0, top_k >= 0, top_p and min_p in [0, 1]")
        seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        # degenerate truncations keep only the top token (custom.py:319-321); min_p 1 keeps the row maximum's class: not degenerate (ties are sampled)
        if T == 0.0 or k == 1 or p == 0.0:
            return KernelArgs(MODE_GREEDY, 0, 0, 1.0, 1.0, 1.0, 0.0, seed)
        temp_first = not self.temperature_last
        inv_temp = 1.0 / T
        filters = (F_TOPK if k > 0 else 0) | (F_TOPP if p < 1.0 else 0) | (F_MINP if mp > 0.0 else 0)
        # min-p before temperature in the stack: ln(min_p); after it: T * ln(min_p) (a threshold on l / T restated on l)
        minp_log = ((T if temp_first else 1.0) * math.log(mp)) if mp > 0.0 else 0.0
        if filters == 0:
            return KernelArgs(MODE_SAMPLE, 0, 0, 1.0, inv_temp, 1.0, 0.0, seed)
        if filters == F_MINP:
            return KernelArgs(MODE_SAMPLE_MINP, 0, 0, 1.0, inv_temp, 1.0, minp_log, seed)
        return KernelArgs(MODE_SAMPLE_FILTERS, filters, k, p, inv_temp, inv_temp if temp_first else 1.0, minp_log, seed)


def workspace_bytes(m: int) -> int:
    """Bytes of the sampler's workspace for m rows (no GPU needed)."""
    n = ctypes.c_int64(0)
    _check(_lib.lib().exl3_sample_workspace(int(m), ctypes.byref(n)))
    return n.value


def workspace(m: int, device) -> torch.Tensor:
    """A zero-filled workspace (the kernels require zeros before the first use and leave zeros behind)."""
    return torch.zeros((workspace_bytes(m) // 8,), dtype=torch.int64, device=device)


def _p(t):
    return None if t is None else t.data_ptr()


def sample(logits: torch.Tensor, settings: SamplerSettings | KernelArgs | None = None, step: torch.Tensor | None = None, *, size: int | None = None,
           row0: int = 0, out: torch.Tensor | None = None, ws: torch.Tensor | None = None, cutoff_out: torch.Tensor | None = None,
           kept_out: torch.Tensor | None = None) -> torch.Tensor:
    """One token per row of fp16 `logits` [m, ld] (m <= 16) -> int32 [m] (-1 for a row holding NaN / +Inf, or nothing above -Inf).  `size`: the unpadded
    vocabulary (columns beyond it are ignored).  `step`: a DEVICE int64 word (None = 0) -- part of the noise counter, read by the kernel, so that a
    captured graph draws fresh noise on every replay; `row0`: the id of the first row in the noise counter.  Graph-capturable when `out` and `ws` are given."""
    ka = settings.kernel_args() if isinstance(settings, SamplerSettings) else (settings or SamplerSettings(temperature=0.0).kernel_args())
    if not (logits.is_cuda and logits.dtype == torch.half and logits.dim() == 2 and logits.is_contiguous()):
        raise RuntimeError("sample: logits must be a contiguous (m, ld) float16 tensor on the GPU")
    m, ld = logits.shape
    if logits.device.index != torch.cuda.current_device():
        torch.cuda.set_device(logits.device)
    if step is not None and not (step.dtype == torch.int64 and step.numel() == 1 and step.device == logits.device):
        raise RuntimeError("sample: step must be one int64 word on the logits' device")
    if out is None:
        out = torch.empty((m,), dtype=torch.int32, device=logits.device)
    if ws is None:
        ws = workspace(m, logits.device)
    for t, dt, nm in ((out, torch.int32, "out"), (cutoff_out, torch.float, "cutoff_out"), (kept_out, torch.int32, "kept_out")):
        if t is not None and not (t.dtype == dt and t.numel() >= m and t.is_contiguous() and t.device == logits.device):
            raise RuntimeError(f"sample: {nm} must hold m contiguous {dt} values on the logits' device")
    _check(_lib.lib().exl3_sample(_p(logits), m, ld, int(ld if size is None else size), ka.mode, ka.filters, ka.top_k, ka.top_p, ka.inv_temp, ka.inv_temp_filter,
                                  ka.minp_log, ka.seed & 0xFFFFFFFF, ka.seed >> 32, _p(step), int(row0), _p(ws), ws.numel() * ws.element_size(), _p(out),
                                  _p(cutoff_out), _p(kept_out), torch.cuda.current_stream(logits.device).cuda_stream))
    return out


def gen_feed(sampled, forced, embed: torch.Tensor, x0: torch.Tensor, tokens_out, positions, cache_seqlens, attn_lens, invalid: torch.Tensor, step: torch.Tensor,
             vocab: int | None = None, *, stop_ids: torch.Tensor | None = None, done: torch.Tensor | None = None, pad_token: int | None = None,
             live: torch.Tensor | None = None):
    """The launch behind the sampler: per row the next token (forced[row, step + 1] while the forced list lasts, else sampled[row]) -> tokens_out[row, step],
    x0[row] = embed[token], the three counters and the step word + 1.  A token outside [0, vocab) leaves x0 alone and sets the sticky invalid[row].
    With stop_ids (int32, <= 64), done (int32 [m], sticky), pad_token and live (one int32 word) the launch is exl3_gen_feed_stop: a row whose SAMPLED token is a
    stop id becomes done -- the token is recorded, not fed; from then on the row's input and counters freeze and tokens_out receives pad_token; live = rows neither
    done nor invalid.  Without them the launch is exl3_gen_feed, unchanged."""
    m, hidden = x0.shape
    ok = embed.dtype == torch.half and x0.dtype == torch.half and embed.is_contiguous() and x0.is_contiguous() and embed.dim() == 2 and embed.shape[1] == hidden
    for t in (sampled, forced, tokens_out, positions, cache_seqlens, attn_lens, invalid):
        ok = ok and (t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.device == x0.device))
    ok = ok and step.dtype == torch.int64 and step.numel() == 1 and invalid.numel() >= m
    ok = ok and (forced is None or (forced.dim() == 2 and forced.shape[0] == m)) and (tokens_out is None or (tokens_out.dim() == 2 and tokens_out.shape[0] == m))
    ok = ok and all(t is None or t.numel() >= m for t in (sampled, positions, cache_seqlens, attn_lens))
    if not ok:
        raise RuntimeError("gen_feed: fp16 embed [vocab, hidden] / x0 [m, hidden], int32 token / counter tensors with m rows, an int64 step word")
    if x0.device.index != torch.cuda.current_device():
        torch.cuda.set_device(x0.device)
    args = (_p(sampled), _p(forced), forced.shape[1] if forced is not None else 0, m, _p(embed), int(embed.shape[0] if vocab is None else vocab),
            hidden, _p(x0), _p(tokens_out), tokens_out.shape[1] if tokens_out is not None else 0, _p(positions), _p(cache_seqlens),
            _p(attn_lens), _p(invalid), _p(step))
    if stop_ids is None and done is None and live is None and pad_token is None:
        _check(_lib.lib().exl3_gen_feed(*args, torch.cuda.current_stream(x0.device).cuda_stream))
        return
    if stop_ids is None or done is None or live is None or pad_token is None:
        raise RuntimeError("gen_feed: stop_ids, done, pad_token and live go together")
    for t, n in ((stop_ids, 0), (done, m), (live, 1)):
        if not (t.dtype == torch.int32 and t.is_contiguous() and t.device == x0.device and t.numel() >= n):
            raise RuntimeError("gen_feed: stop_ids / done [m] / live [1] must be contiguous int32 tensors on the device of x0")
    _check(_lib.lib().exl3_gen_feed_stop(*args, _p(stop_ids), stop_ids.numel(), _p(done), int(pad_token), _p(live), torch.cuda.current_stream(x0.device).cuda_stream))


def embed_rows(ids: torch.Tensor, col0: int, T: int, embed: torch.Tensor, invalid: torch.Tensor, vocab: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """The input rows of a prefill chunk: out[b * T + t] = embed[ids[b, col0 + t]] for the int32 id matrix `ids` [m, ld] (m <= 16) on the device -> fp16
    [m * T, hidden].  An id outside [0, vocab) never indexes the table: its row is zeros and the sticky invalid[b] is set.  One launch (exl3_embed_rows),
    graph-capturable when `out` is given."""
    ok = (ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 2 and ids.is_contiguous() and embed.dtype == torch.half and embed.dim() == 2
          and embed.is_contiguous() and embed.device == ids.device and invalid.dtype == torch.int32 and invalid.is_contiguous() and invalid.device == ids.device
          and invalid.numel() >= ids.shape[0])
    if not ok:
        raise RuntimeError("embed_rows: contiguous int32 ids [m, ld] and invalid [m], fp16 embed [vocab, hidden], all on one GPU")
    m, ld = ids.shape
    hidden = embed.shape[1]
    if out is None:
        out = torch.empty((m * int(T), hidden), dtype=torch.half, device=ids.device)
    if not (out.dtype == torch.half and out.is_contiguous() and out.device == ids.device and out.numel() == m * int(T) * hidden):
        raise RuntimeError("embed_rows: out must be a contiguous fp16 [m * T, hidden] tensor on the ids' device")
    if ids.device.index != torch.cuda.current_device():
        torch.cuda.set_device(ids.device)
    _check(_lib.lib().exl3_embed_rows(_p(ids), ld, int(col0), int(T), m, _p(embed), int(embed.shape[0] if vocab is None else vocab), hidden, _p(out), _p(invalid),
                                      torch.cuda.current_stream(ids.device).cuda_stream))
    return out


MAX_STOP_IDS = 64
_F32_MAX = float(torch.finfo(torch.float32).max)


class LogitProcessors:
    """What exl3_logit_process applies to a row of logits, in this order: repetition penalty (rep_p; 1 = off) and presence / frequency penalties (pres_p, freq_p;
    0 = off) over the past tokens, each with its own (sustain, decay) window as in the reference (custom.py: SS_RepP, SS_PresFreqP); logit_bias {id: value}
    (-inf bans) with ban_token_ids folded in as -inf; bitmask: an int32 / uint32 tensor [1 or m][words], bit set = keep (apply_logit_bitmask's layout) -- a tensor
    already on the device is used where it lies, so a grammar filter may rewrite it between replays.
    No-ops collapse by the reference's rules: rep_p == 1 or sustain + decay <= 0 switches the repetition penalty off (custom.py:790-793), pres_p == freq_p == 0
    or sustain + decay <= 0 the other (:855-858); bias entries that are 0, NaN or overflow fp32 to +inf are dropped (:586-595); ids outside the vocabulary are
    ignored.  The device tensors are built once per (vocabulary, device)."""

    def __init__(self, rep_p: float = 1.0, rep_sustain: int = 10 ** 8, rep_decay: int = 0, pres_p: float = 0.0, freq_p: float = 0.0, pf_sustain: int = 10 ** 8,
                 pf_decay: int = 0, logit_bias: dict | None = None, ban_token_ids=None, bitmask: torch.Tensor | None = None):
        rep_p, pres_p, freq_p = float(rep_p), float(pres_p), float(freq_p)
        if not (math.isfinite(rep_p) and rep_p > 0.0 and math.isfinite(pres_p) and math.isfinite(freq_p)):
            raise ValueError("LogitProcessors: rep_p must be positive and finite, pres_p and freq_p finite")
        for nm, v in (("rep_sustain", rep_sustain), ("rep_decay", rep_decay), ("pf_sustain", pf_sustain), ("pf_decay", pf_decay)):
            if int(v) != v or not (0 <= int(v) < 2 ** 31):
                raise ValueError(f"LogitProcessors: {nm} must be an integer in [0, 2^31)")
        if int(rep_sustain) + int(rep_decay) >= 2 ** 31 or int(pf_sustain) + int(pf_decay) >= 2 ** 31:
            raise ValueError("LogitProcessors: sustain + decay must fit an int32")
        self.rep_on = rep_p != 1.0 and int(rep_sustain) + int(rep_decay) > 0
        self.pf_on = (pres_p != 0.0 or freq_p != 0.0) and int(pf_sustain) + int(pf_decay) > 0
        # a penalty that is off reaches the kernel as its neutral element
        self.rep_p, self.rep_sustain, self.rep_decay = (rep_p, int(rep_sustain), int(rep_decay)) if self.rep_on else (1.0, 0, 0)
        self.pres_p, self.freq_p, self.pf_sustain, self.pf_decay = (pres_p, freq_p, int(pf_sustain), int(pf_decay)) if self.pf_on else (0.0, 0.0, 0, 0)
        bias = {}
        for t, v in (logit_bias or {}).items():
            v = float(v)
            if v != 0.0 and v == v and v <= _F32_MAX:
                bias[int(t)] = v
        for t in (ban_token_ids if ban_token_ids is not None else ()):
            bias[int(t)] = float("-inf")
        self.bias = bias
        if bitmask is not None:
            if not (isinstance(bitmask, torch.Tensor) and bitmask.dtype in (torch.int32, torch.uint32) and bitmask.dim() == 2 and bitmask.shape[1] >= 1
                    and bitmask.is_contiguous()):
                raise ValueError("LogitProcessors: bitmask must be a contiguous int32 / uint32 tensor [1 or m][words]")
        self.bitmask = bitmask
        self._vectors = {}

    @property
    def needs_history(self) -> bool:
        return self.rep_on or self.pf_on

    @property
    def is_noop(self) -> bool:
        return not (self.rep_on or self.pf_on or self.bias or self.bitmask is not None)

    def tensors(self, vocab: int, device):
        """(bias fp32 [vocab] or None, bitmask on `device` or None), cached per (vocab, device)."""
        device = torch.device(device)
        key = (int(vocab), device)
        got = self._vectors.get(key)
        if got is None:
            items = [(t, v) for t, v in self.bias.items() if 0 <= t < vocab]
            vec = None
            if items:
                vec = torch.zeros((vocab,), dtype=torch.float)
                vec[torch.tensor([t for t, _ in items], dtype=torch.long)] = torch.tensor([v for _, v in items], dtype=torch.float)
                vec = vec.to(device)
            bm = self.bitmask
            if bm is not None and bm.device != device:
                bm = bm.to(device)
            got = self._vectors[key] = (vec, bm)
        return got


def process_logits(logits: torch.Tensor, procs: LogitProcessors, past_a: torch.Tensor | None = None, past_b: torch.Tensor | None = None, len_b: int | None = None,
                   step: torch.Tensor | None = None, *, size: int | None = None, len_b_bias: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """procs applied to fp16 / fp32 `logits` [m, ld] (m <= 16) -> `out` (fp16 / fp32, default: a new tensor of the input's type; may be `logits` itself).  The past
    ids of row r are past_a[r, :] followed by past_b[r, :len_b], int32 (past_a may be a column view such as forced[:, 0:1]); the length of the second segment is
    the host integer len_b (default: all of past_b) or, with `step` (a DEVICE int64 word), clamp(step + len_b_bias, 0, past_b.shape[1]) read by the kernel.  One
    launch, graph-capturable when `out` is given (the bias vector is built at the first call for a vocabulary: call once outside the capture)."""
    if not (logits.is_cuda and logits.dtype in (torch.half, torch.float) and logits.dim() == 2 and logits.is_contiguous()):
        raise RuntimeError("process_logits: logits must be a contiguous (m, ld) float16 / float32 tensor on the GPU")
    m, ld = logits.shape
    size = int(ld if size is None else size)
    if out is None:
        out = torch.empty_like(logits)
    if not (out.is_cuda and out.device == logits.device and out.dtype in (torch.half, torch.float) and out.shape == logits.shape and out.is_contiguous()):
        raise RuntimeError("process_logits: out must be a contiguous float16 / float32 tensor of the logits' shape on their device")
    seg = []
    for t, nm in ((past_a, "past_a"), (past_b, "past_b")):
        if t is None:
            seg.append((None, 0, 0))
            continue
        if not (t.dtype == torch.int32 and t.dim() == 2 and t.shape[0] == m and t.device == logits.device and (t.shape[1] == 0 or t.stride(1) == 1)):
            raise RuntimeError(f"process_logits: {nm} must be an int32 [m, n] tensor on the logits' device with unit column stride")
        ldt = t.stride(0) if (m > 1 and t.shape[1] > 0) else t.shape[1]
        if ldt < t.shape[1]:
            raise RuntimeError(f"process_logits: rows of {nm} overlap")
        seg.append((t.data_ptr() if t.shape[1] > 0 else None, int(ldt), int(t.shape[1])))
    (pa, lda, len_a), (pb, ldb, cap_b) = seg
    if step is not None:
        if not (step.dtype == torch.int64 and step.numel() == 1 and step.device == logits.device):
            raise RuntimeError("process_logits: step must be one int64 word on the logits' device")
        if past_b is None or len_b is not None or ldb != cap_b:
            raise RuntimeError("process_logits: the device length needs a contiguous past_b and no host len_b")
        lb = 0
    else:
        lb = cap_b if len_b is None else int(len_b)
        if not (0 <= lb <= cap_b):
            raise RuntimeError("process_logits: len_b outside past_b")
    bias, bm = procs.tensors(size, logits.device)
    if bm is not None and bm.shape[0] not in (1, m):
        raise RuntimeError("process_logits: the bitmask has 1 or m rows")
    if logits.device.index != torch.cuda.current_device():
        torch.cuda.set_device(logits.device)
    _check(_lib.lib().exl3_logit_process(_p(logits), int(logits.dtype == torch.float), _p(out), int(out.dtype == torch.float), m, ld, size,
                                         pa, lda, len_a, pb, ldb, lb, _p(step), int(len_b_bias),
                                         procs.rep_p, procs.rep_sustain, procs.rep_decay, procs.pres_p, procs.freq_p, procs.pf_sustain, procs.pf_decay,
                                         _p(bias), _p(bm), 0 if bm is None else bm.shape[0], 0 if bm is None else bm.shape[1],
                                         torch.cuda.current_stream(logits.device).cuda_stream))
    return out


# ---- speculative decoding (csrc/exl3_spec.hip) -------------------------------------------------------------------------------------------------------------
SPEC_BASE, SPEC_PRODUCED, SPEC_LIVE, SPEC_DONE, SPEC_INVALID, SPEC_NDRAFT, SPEC_ROUNDS, SPEC_DRAFTED, SPEC_ACCEPTED = range(9)
SPEC_STATE_WORDS = 9           # include/exl3_hip.h EXL3_SPEC_STATE_WORDS
SPEC_MAX_MATCH = 16


@dataclass(frozen=True)
class SpeculativeSettings:
    """Speculative decoding in generate(): num_draft_tokens drafts per verify step (the step runs num_draft_tokens + 1 rows, so at most 15).  The drafts come
    from the n-gram matcher over the sequence's own history (the longest suffix of ngram_match_min .. ngram_match_max tokens that occurred before, continued
    the way it continued then) or, with script (token ids by ABSOLUTE position, -1 = no draft from here; shorter than the context: padded with -1), from that
    table -- the seam for a host-side or draft-model drafter, and how tests force acceptance patterns.  The drafts never change the output, only the number
    of verify steps it takes.  The default of 3 drafts: m = 4 is the widest batch of the 1-4-row GEMV generation."""
    num_draft_tokens: int = 3
    ngram_match_min: int = 2
    ngram_match_max: int = 8
    script: object = None

    def __post_init__(self):
        k, lo, hi = int(self.num_draft_tokens), int(self.ngram_match_min), int(self.ngram_match_max)
        if not (1 <= k <= MAX_ROWS - 1):
            raise ValueError("SpeculativeSettings: num_draft_tokens must be in [1, 15]")
        if not (1 <= lo <= hi <= SPEC_MAX_MATCH):
            raise ValueError("SpeculativeSettings: 1 <= ngram_match_min <= ngram_match_max <= 16")


def _spec_check(name, x0, embed, int_tensors, state, m):
    ok = (x0.is_cuda and x0.dtype == torch.half and x0.dim() == 2 and x0.is_contiguous() and embed.dtype == torch.half and embed.dim() == 2 and embed.is_contiguous()
          and embed.shape[1] == x0.shape[1] and embed.device == x0.device)
    for t, n in int_tensors:
        ok = ok and (t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.device == x0.device and t.numel() >= n))
    ok = ok and state.numel() >= SPEC_STATE_WORDS and 1 <= m <= MAX_ROWS
    if not ok:
        raise RuntimeError(f"{name}: fp16 embed [vocab, hidden] / x0 [m, hidden] (m <= 16), contiguous int32 tensors on the device of x0, a state of {SPEC_STATE_WORDS} words")
    if x0.device.index != torch.cuda.current_device():
        torch.cuda.set_device(x0.device)


def spec_accept(sampled: torch.Tensor, in_tokens: torch.Tensor, state: torch.Tensor, round_word: torch.Tensor, hist: torch.Tensor, tokens_out: torch.Tensor,
                vocab: int, stop_ids: torch.Tensor | None = None, max_new: int | None = None):
    """exl3_spec_accept: the launch behind the sampler of a verify step -- commits the drafts that equal the target's own tokens and the one token behind them
    (sampled[0 .. n] -> hist and tokens_out), advances base / produced / round and the counters in `state` (int32 [SPEC_STATE_WORDS]); max_new defaults
    to tokens_out.numel().  Stop ids, the budget and an out-of-vocabulary sample cut the run (include/exl3_hip.h)."""
    m = in_tokens.numel()
    ok = all(t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda and t.device == state.device for t in (sampled, in_tokens, state, hist, tokens_out))
    ok = ok and (stop_ids is None or (stop_ids.dtype == torch.int32 and stop_ids.is_contiguous() and stop_ids.device == state.device))
    max_new = tokens_out.numel() if max_new is None else int(max_new)
    ok = ok and sampled.numel() >= m and 0 <= max_new <= tokens_out.numel() and state.numel() >= SPEC_STATE_WORDS and round_word.dtype == torch.int64 and round_word.numel() == 1 and round_word.device == state.device
    if not ok:
        raise RuntimeError("spec_accept: contiguous int32 sampled / in_tokens [m] / state / hist / tokens_out / stop_ids and an int64 round word on one GPU")
    if state.device.index != torch.cuda.current_device():
        torch.cuda.set_device(state.device)
    _check(_lib.lib().exl3_spec_accept(_p(sampled), _p(in_tokens), m, int(vocab), _p(state), _p(round_word), _p(hist), hist.numel(), _p(tokens_out), max_new,
                                       _p(stop_ids), 0 if stop_ids is None else stop_ids.numel(), torch.cuda.current_stream(state.device).cuda_stream))


def spec_draft(hist: torch.Tensor, state: torch.Tensor, in_tokens: torch.Tensor, embed: torch.Tensor, x0: torch.Tensor, positions: torch.Tensor,
               cache_seqlens: torch.Tensor, attn_lens: torch.Tensor, k: int, max_new: int, match_min: int = 2, match_max: int = 8,
               script: torch.Tensor | None = None, vocab: int | None = None):
    """exl3_spec_draft_ngram: up to k drafts behind the committed history hist[0 .. base] (n-gram match, or script[base + 1 ..] when a script is given) and the
    inputs of the next verify step: in_tokens [m], state's n_draft, positions / cache_seqlens / attn_lens [m] and x0 [m, hidden] = embed[in_tokens]."""
    m = x0.shape[0]
    _spec_check("spec_draft", x0, embed, ((hist, 1), (state, SPEC_STATE_WORDS), (in_tokens, m), (positions, m), (cache_seqlens, m), (attn_lens, m), (script, hist.numel())),
                state, m)
    _check(_lib.lib().exl3_spec_draft_ngram(_p(hist), hist.numel(), _p(script), int(k), int(match_min), int(match_max), m, _p(state), int(max_new), _p(in_tokens),
                                            _p(embed), int(embed.shape[0] if vocab is None else vocab), x0.shape[1], _p(x0), _p(positions), _p(cache_seqlens),
                                            _p(attn_lens), torch.cuda.current_stream(x0.device).cuda_stream))


def spec_round(sampled: torch.Tensor, in_tokens: torch.Tensor, state: torch.Tensor, round_word: torch.Tensor, hist: torch.Tensor, tokens_out: torch.Tensor,
               embed: torch.Tensor, x0: torch.Tensor, positions: torch.Tensor, cache_seqlens: torch.Tensor, attn_lens: torch.Tensor, k: int, match_min: int = 2,
               match_max: int = 8, script: torch.Tensor | None = None, stop_ids: torch.Tensor | None = None, vocab: int | None = None, max_new: int | None = None):
    """exl3_spec_round: spec_accept followed by spec_draft in ONE launch (max_new defaults to tokens_out.numel())."""
    m = x0.shape[0]
    max_new = tokens_out.numel() if max_new is None else int(max_new)
    if not (0 <= max_new <= tokens_out.numel()):
        raise RuntimeError("spec_round: max_new outside tokens_out")
    _spec_check("spec_round", x0, embed, ((sampled, m), (hist, 1), (state, SPEC_STATE_WORDS), (in_tokens, m), (tokens_out, 0), (positions, m), (cache_seqlens, m),
                                          (attn_lens, m), (script, hist.numel()), (stop_ids, 0)), state, m)
    if not (round_word.dtype == torch.int64 and round_word.numel() == 1 and round_word.device == x0.device):
        raise RuntimeError("spec_round: the round word must be one int64 word on the device of x0")
    _check(_lib.lib().exl3_spec_round(_p(sampled), _p(in_tokens), m, int(embed.shape[0] if vocab is None else vocab), _p(state), _p(round_word), _p(hist), hist.numel(),
                                      _p(tokens_out), max_new, _p(stop_ids), 0 if stop_ids is None else stop_ids.numel(), _p(script), int(k),
                                      int(match_min), int(match_max), _p(embed), x0.shape[1], _p(x0), _p(positions), _p(cache_seqlens), _p(attn_lens),
                                      torch.cuda.current_stream(x0.device).cuda_stream))
