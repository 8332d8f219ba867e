"""Length regulator: phoneme states and integer durations to frame states, with its gradient.

The operator a non-autoregressive student (FastSpeech / FastSpeech 2) needs between its phoneme-rate
and its frame-rate halves, over the three kernels of csrc/regulate.hip (include/tt2_capi.h has the
definition):

* ``plan(durations, text_len, max_frames)``: segment ends, the frame -> phoneme index and the frame
  counts of a batch (tt2_regulate_plan).  With ``max_frames`` given nothing synchronises with the
  host, so the call can be captured into a graph.
* ``length_regulate(h, durations | plan=)``: ``out[b, n] = h[b, index[b, n]]``, zeros past an
  utterance's frames; differentiable in ``h`` (forward tt2_regulate_fwd, backward tt2_regulate_bwd).
* ``segment_sum(values, plan)``: the sum of frame values per phoneme, the transpose of the
  expansion; differentiable in ``values`` (forward tt2_regulate_bwd, backward tt2_regulate_fwd).
  ``segment_sum(v, p) / d`` is the plain mean per phoneme; masked means are ``phoneme_average``'s.
* ``LengthRegulator``: the nn.Module over ``length_regulate``.
* ``round_durations``: a duration predictor's log-domain output to integer frames (pure torch).

The durations are what ``tt2.data.extract_durations`` writes (``Durations.durations``,
``MonotonicAlignment.durations``); the index of their plan is ``MonotonicAlignment.path``.  Both
gradients are bit-identical run to run: a phoneme's gradient is the f32 sum of its frames' in
ascending frame order, rounded once.  Every result is a fresh tensor outside any arena.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops
from ._lib import REGULATE_MAX_PHONEMES

INT32_MAX = 2 ** 31 - 1


class RegulatorPlan(NamedTuple):
    """plan(): index [B, n_out] int32 (the phoneme of each frame, -1 past the utterance), ends
    [B, Tx] int32 (the clamped running sum of the durations), frames [B] int32 (frames written per
    utterance), total [B] int32 (frames asked for: total > frames where max_frames cut it)."""
    index: torch.Tensor
    ends: torch.Tensor
    frames: torch.Tensor
    total: torch.Tensor


class Regulated(NamedTuple):
    """length_regulate(): out [B, n_out, D] (or [B, n_out]), frames [B] int32, index [B, n_out] int32."""
    out: torch.Tensor
    frames: torch.Tensor
    index: torch.Tensor


def _lens32(who, text_len, B, dev):
    if text_len is None:
        return None
    if text_len.dim() != 1 or text_len.shape[0] != B or text_len.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: text_len must be an integer [{B}], got {text_len.dtype} {tuple(text_len.shape)}")
    return text_len.to(device=dev, dtype=torch.int32).contiguous()


def plan(durations: torch.Tensor, text_len: torch.Tensor | None = None, max_frames: int | None = None) -> RegulatorPlan:
    """durations [B, Tx] int32 or int64 on the GPU (negatives count as 0), text_len [B] (phonemes
    per utterance; durations at and past it are ignored) -> RegulatorPlan with n_out = max_frames.
    With max_frames given there is no host synchronisation and utterances longer than it are cut
    (plan.total > plan.frames shows which).  With max_frames None the call runs the plan once with
    n_out = 0, reads the largest total on the host -- one synchronisation -- and sizes the output to
    it."""
    who = "regulate.plan"
    if durations.dim() != 2 or durations.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: durations must be an integer [B, Tx], got {durations.dtype} {tuple(durations.shape)}")
    if not durations.is_cuda:
        raise ValueError(f"{who}: durations must be on the GPU")
    B, Tx = durations.shape
    if Tx > REGULATE_MAX_PHONEMES:
        raise ValueError(f"{who}: Tx = {Tx} above TT2_REGULATE_MAX_PHONEMES = {REGULATE_MAX_PHONEMES}")
    if max_frames is not None and not (0 <= int(max_frames) <= INT32_MAX):
        raise ValueError(f"{who}: max_frames must be in [0, 2^31 - 1], got {max_frames}")
    dev = durations.device
    if durations.dtype == torch.int64:
        durations = durations.clamp(-1, INT32_MAX)
    d32 = durations.to(torch.int32)
    if Tx > 1 and d32.stride(1) != 1:
        d32 = d32.contiguous()
    lens = _lens32(who, text_len, B, dev)
    ends = torch.empty(B, Tx, dtype=torch.int32, device=dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    total = torch.empty(B, dtype=torch.int32, device=dev)
    if max_frames is None:
        if B == 0:
            n_out = 0
        else:
            ops.regulate_plan(d32, 0, key_len=lens, ends=ends, total=total)
            n_out = int(total.max().item())     # the one host synchronisation
    else:
        n_out = int(max_frames)
    index = torch.empty(B, n_out, dtype=torch.int32, device=dev)
    ops.regulate_plan(d32, n_out, key_len=lens, ends=ends, index=index, frames=frames, total=total)
    return RegulatorPlan(index, ends, frames, total)


_make_plan = plan      # length_regulate has a parameter of that name


class _Expand(torch.autograd.Function):
    """y = h[index]: forward tt2_regulate_fwd, backward tt2_regulate_bwd."""

    @staticmethod
    def forward(ctx, h, index, ends):
        y = torch.empty(h.shape[0], index.shape[1], h.shape[2], dtype=h.dtype, device=h.device)
        ops.regulate_fwd(h, index, y)
        ctx.save_for_backward(ends)
        ctx.tx = h.shape[1]
        return y

    @staticmethod
    def backward(ctx, dy):
        (ends,) = ctx.saved_tensors
        dy = dy.contiguous()      # a gradient can arrive expanded (stride 0)
        dh = torch.empty(dy.shape[0], ctx.tx, dy.shape[2], dtype=dy.dtype, device=dy.device)
        ops.regulate_bwd(dy, ends, dh)
        return dh, None, None


class _SegmentSum(torch.autograd.Function):
    """s = the sum of v over each phoneme's frames: forward tt2_regulate_bwd, backward tt2_regulate_fwd."""

    @staticmethod
    def forward(ctx, v, index, ends):
        s = torch.empty(v.shape[0], ends.shape[1], v.shape[2], dtype=v.dtype, device=v.device)
        ops.regulate_bwd(v, ends, s)
        ctx.save_for_backward(index)
        return s

    @staticmethod
    def backward(ctx, ds):
        (index,) = ctx.saved_tensors
        ds = ds.contiguous()
        dv = torch.empty(ds.shape[0], index.shape[1], ds.shape[2], dtype=ds.dtype, device=ds.device)
        ops.regulate_fwd(ds, index, dv)
        return dv, None, None


def _rows3(who, name, x, B, rows):
    """[B, rows] or [B, rows, D], f32 or bf16, on the GPU -> ([B, rows, D] view, was_2d)."""
    if x.dim() not in (2, 3) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda:
        raise ValueError(f"{who}: {name} must be f32 or bf16 [B, T] or [B, T, D] on the GPU, got {x.dtype} {tuple(x.shape)}")
    if x.shape[0] != B or x.shape[1] != rows:
        raise ValueError(f"{who}: {name} is {tuple(x.shape)}, the plan is for [{B}, {rows}]")
    flat = x.dim() == 2
    x3 = x.unsqueeze(2) if flat else x
    if x3.shape[2] > 1 and x3.stride(2) != 1:
        x3 = x3.contiguous()
    return x3, flat


def length_regulate(h: torch.Tensor, durations: torch.Tensor | None = None, text_len: torch.Tensor | None = None,
                    max_frames: int | None = None, plan: RegulatorPlan | None = None) -> Regulated:
    """h [B, Tx, D] or [B, Tx], f32 or bf16 -> Regulated(out [B, n_out, D] or [B, n_out], frames,
    index): out[b, n] = h[b, index[b, n]] (the bits, copied) and +0 for n >= frames[b].  Give either
    durations (with text_len and max_frames as in plan()) or a plan made before: a plan is reusable
    across calls (the hidden states, then pitch and energy).  Differentiable in h: a phoneme's
    gradient is the f32 sum of its frames' gradients in ascending frame order, rounded once --
    bit-identical run to run.  With max_frames or plan= there is no host synchronisation."""
    who = "length_regulate"
    if (durations is None) == (plan is None):
        raise ValueError(f"{who}: give durations or plan=, not both")
    if plan is None:
        plan = _make_plan(durations, text_len, max_frames)
    elif text_len is not None or max_frames is not None:
        raise ValueError(f"{who}: text_len and max_frames belong to the plan")
    h3, flat = _rows3(who, "h", h, plan.ends.shape[0], plan.ends.shape[1])
    y = _Expand.apply(h3, plan.index, plan.ends)
    return Regulated(y.squeeze(2) if flat else y, plan.frames, plan.index)


def segment_sum(values: torch.Tensor, plan: RegulatorPlan) -> torch.Tensor:
    """values [B, n_out, D] or [B, n_out], f32 or bf16 -> [B, Tx, D] or [B, Tx]: the sum of each
    phoneme's frames, added in f32 in ascending frame order and rounded once; +0 for a phoneme
    without frames.  Frames at and past plan.frames[b] are not read.  Differentiable in values (the
    gradient is the expansion).  No host synchronisation."""
    v3, flat = _rows3("segment_sum", "values", values, plan.index.shape[0], plan.index.shape[1])
    s = _SegmentSum.apply(v3, plan.index, plan.ends)
    return s.squeeze(2) if flat else s


class LengthRegulator(torch.nn.Module):
    """forward(h, durations, text_len=None, max_frames=None) -> Regulated; see length_regulate.  No
    parameters."""

    def forward(self, h, durations, text_len=None, max_frames=None):
        return length_regulate(h, durations, text_len=text_len, max_frames=max_frames)


def round_durations(log_d: torch.Tensor, text_len: torch.Tensor | None = None, alpha: float = 1.0,
                    min_frames: int = 0) -> torch.Tensor:
    """A duration predictor's output to integer frames: log_d [B, Tx] = log(d + 1) ->
    d = clamp(round_half_even(alpha * max(exp(log_d) - 1, 0)), min_frames, 2^31 - 1) as int32, and 0
    at and past text_len[b].  Conventions differ between implementations (log(d) against log(d + 1),
    round against ceil or floor, whether alpha scales before or after rounding, a floor of 0 or 1
    frame); this is the FastSpeech / ESPnet inference convention (targets log(d + 1),
    round(exp(x) - 1) with torch.round's ties to even, alpha applied before rounding, min_frames = 0),
    and min_frames = 1 gives the variant that never drops a phoneme.  Pure torch, in f32 (f64 for an
    f64 input); a NaN prediction gives min_frames.  No host synchronisation."""
    if log_d.dim() != 2 or not log_d.is_floating_point():
        raise ValueError(f"round_durations: log_d must be a floating-point [B, Tx], got {log_d.dtype} {tuple(log_d.shape)}")
    if not (0 <= int(min_frames) <= INT32_MAX) or not alpha >= 0.0:
        raise ValueError(f"round_durations: min_frames in [0, 2^31 - 1] and alpha >= 0, got {min_frames}, {alpha}")
    x = log_d.double() if log_d.dtype == torch.float64 else log_d.float()
    d = torch.round(float(alpha) * torch.clamp(torch.exp(x) - 1.0, min=0.0))
    d = torch.nan_to_num(d, nan=0.0).double().clamp(float(int(min_frames)), float(INT32_MAX)).to(torch.int64)
    if text_len is not None:
        lens = _lens32("round_durations", text_len, log_d.shape[0], log_d.device)
        t = torch.arange(log_d.shape[1], device=log_d.device)
        d = torch.where(t[None, :] < lens[:, None], d, torch.zeros_like(d))
    return d.to(torch.int32)
