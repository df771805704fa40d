"""
Device-side sampling (csrc/exl3_sampler.hip; include/exl3_hip.h: exl3_sample / exl3_gen_feed).

SamplerSettings collapses a (temperature, top-k, top-p, min-p) stack into the kernel's (mode, filters, ...) the way the reference collapses a sampler
stack into its fused sampler (generator/sampler/custom.py:267-343): greedy when nothing can change the top token, a Gumbel sample of softmax(l / T)
otherwise, restricted to one cutoff for min-p alone (mode 2) or for any combination with top-k / top-p (mode 3).

The noise is this library's own Philox4x32-10 stream keyed by (seed; column, row, step) -- NOT curand's sequence, so the reference's op names
(argmax_sample, gumbel_sample, fused_sampler, gumbel_noise_*) are deliberately absent from exllamav3_amd.ext.
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
             vocab: int | None = None):
    """The launch behind the sampler: per row the next token (forced[row, step + 1] while the forced list lasts, else sampled[row]) -> tokens_out[row, step],
    x0[row] = embed[token], the three counters and the step word + 1.  A token outside [0, vocab) leaves x0 alone and sets the sticky invalid[row]."""
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
    _check(_lib.lib().exl3_gen_feed(_p(sampled), _p(forced), forced.shape[1] if forced is not None else 0, m, _p(embed), int(embed.shape[0] if vocab is None else vocab),
                                    hidden, _p(x0), _p(tokens_out), tokens_out.shape[1] if tokens_out is not None else 0, _p(positions), _p(cache_seqlens),
                                    _p(attn_lens), _p(invalid), _p(step), torch.cuda.current_stream(x0.device).cuda_stream))
