"""Gaussian upsampling: the soft length regulator, differentiable in the states, the durations and the
widths.

Where ``regulate.length_regulate`` repeats a phoneme's state for its frames, Gaussian upsampling
(Non-Attentive Tacotron, Parallel Tacotron; ESPnet's ``GaussianUpsampling`` in JETS and VITS) gives
frame n a softmax-weighted mean of the phoneme states, the weight of phoneme t falling off with the
squared distance between the frame and the phoneme's centre.  Over the two kernels of
csrc/upsample.hip (include/tt2_capi.h has the definition), which never write the [frames, phonemes]
weight matrix, forward or backward:

* ``centers(durations, text_len)``: ``cumsum(d) - d / 2`` in f32 (pure torch, differentiable).
* ``gaussian_upsample(h, durations, ...)``: ``out[b, n] = sum_t softmax_t(e[n, t]) h[b, t]`` with
  ``e[n, t] = -delta (n + offset - c_t)^2`` (ESPnet's form) or, with ``sigma=``,
  ``e[n, t] = -ln sigma_t - (n + offset - c_t)^2 / (2 sigma_t^2)`` (Non-Attentive Tacotron's).
  Differentiable in ``h``, in floating ``durations`` and in tensor ``delta`` / ``sigma``; the kernel is
  asked only for the gradients autograd needs, and all of them are bit-identical run to run.
* ``GaussianUpsampling``: the nn.Module over it.

The durations are what ``forward_sum.best_path`` and ``tt2.data.extract_durations`` write.  The one
difference from ESPnet: its frames past an utterance's length hold the softmax row of a fully masked
line (the state of phoneme 0, or NaN); here they are exactly +0, as with ``length_regulate``.  Every
result is a fresh tensor outside any arena.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops
from ._lib import REGULATE_MAX_PHONEMES, UPSAMPLE_MAX_DIM

INT32_MAX = 2 ** 31 - 1
DEFAULT_DELTA = 0.1


class Upsampled(NamedTuple):
    """gaussian_upsample(): out [B, n_out, D] (or [B, n_out]), frames [B] int32 (the frames of each
    utterance; rows of out at and past it are +0)."""
    out: torch.Tensor
    frames: torch.Tensor


def _lens32(who, name, lens, B, dev):
    if lens is None:
        return None
    if lens.dim() != 1 or lens.shape[0] != B or lens.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: {name} must be an integer [{B}], got {lens.dtype} {tuple(lens.shape)}")
    return lens.to(device=dev, dtype=torch.int32).contiguous()


def _durations(who, durations):
    if durations.dim() != 2 or durations.dtype not in (torch.int32, torch.int64, torch.float32, torch.float64,
                                                       torch.bfloat16, torch.float16):
        raise ValueError(f"{who}: durations must be an integer or floating [B, Tx], got {durations.dtype} {tuple(durations.shape)}")


def _valid(lens, Tx, dev):
    return torch.arange(Tx, device=dev)[None, :] < lens[:, None]


def centers(durations: torch.Tensor, text_len: torch.Tensor | None = None) -> torch.Tensor:
    """durations [B, Tx], integer (as best_path and extract_durations write them) or floating ->
    the phonemes' centres ``cumsum(d) - d / 2`` as f32 [B, Tx], and 0 at and past text_len[b].  Pure
    torch; differentiable for floating durations.  No host synchronisation."""
    who = "upsample.centers"
    _durations(who, durations)
    d = durations.to(torch.float32)
    c = torch.cumsum(d, dim=1) - 0.5 * d
    if text_len is not None:
        lens = _lens32(who, "text_len", text_len, durations.shape[0], durations.device)
        c = torch.where(_valid(lens, durations.shape[1], durations.device), c, torch.zeros_like(c))
    return c


class _GaussUp(torch.autograd.Function):
    """y = softmax(e) h: forward tt2_gauss_upsample_fwd, backward tt2_gauss_upsample_bwd."""

    @staticmethod
    def forward(ctx, h, center, prec, bias, frames, lens, n_out, offset):
        B, _, D = h.shape
        y = torch.empty(B, n_out, D, dtype=h.dtype, device=h.device)
        lse = torch.empty(B, n_out, dtype=torch.float32, device=h.device)
        ops.gauss_upsample_fwd(h, center, prec, y, lse, bias=bias, q_len=frames, key_len=lens, offset=offset)
        ctx.save_for_backward(h, center, prec, bias, frames, lens, y, lse)
        ctx.offset = offset
        return y

    @staticmethod
    def backward(ctx, dy):
        h, center, prec, bias, frames, lens, y, lse = ctx.saved_tensors
        need_h, need_c, need_p, need_b = ctx.needs_input_grad[:4]
        need_b = need_b and bias is not None
        if not (need_h or need_c or need_p or need_b):
            return (None,) * 8
        dy = dy.contiguous()      # a gradient can arrive expanded (stride 0)
        vec = lambda need: torch.empty_like(center) if need else None     # noqa: E731
        dh = torch.empty_like(h, memory_format=torch.contiguous_format) if need_h else None
        dc, dp, db = vec(need_c), vec(need_p), vec(need_b)
        ops.gauss_upsample_bwd(h, center, prec, y, lse, dy, dh=dh, dcenter=dc, dprec=dp, dbias=db, bias=bias,
                               q_len=frames, key_len=lens, offset=ctx.offset)
        return dh, dc, dp, db, None, None, None, None


def gaussian_upsample(h: torch.Tensor, durations: torch.Tensor, text_len: torch.Tensor | None = None,
                      mel_len: torch.Tensor | None = None, max_frames: int | None = None,
                      delta: float | torch.Tensor = DEFAULT_DELTA, sigma: torch.Tensor | None = None,
                      offset: float = 0.0) -> Upsampled:
    """h [B, Tx, D] or [B, Tx], f32 or bf16, durations [B, Tx] (integer or floating) ->
    Upsampled(out [B, n_out, D] or [B, n_out], frames [B] int32).

    ``out[b, n] = sum_t W[n, t] h[b, t]``, W[n, .] the softmax over t < text_len[b] of
    ``-delta (n + offset - c_t)^2`` with ``c = centers(durations, text_len)``; delta is a float or a
    [B, Tx] tensor (ESPnet: delta = 0.1, offset = 0).  sigma, a [B, Tx] tensor of positive widths,
    selects Non-Attentive Tacotron's form instead, ``-ln sigma_t - (n + offset - c_t)^2 / (2 sigma_t^2)``
    (its offset is 1); giving both a non-default delta and sigma is an error.

    frames is mel_len if given, else ``clamp(round(sum_t d), 0, n_out)`` computed on the device; rows
    of out at and past frames[b] are +0.  n_out is max_frames if given -- then nothing synchronises
    with the host and the call can be captured into a graph -- else the largest mel_len or frame count,
    read once on the host: the one synchronisation.

    Differentiable in h, in floating durations and in tensor delta / sigma; only the gradients
    autograd needs are computed, each bit-identical run to run."""
    who = "gaussian_upsample"
    if h.dim() not in (2, 3) or h.dtype not in (torch.float32, torch.bfloat16) or not h.is_cuda:
        raise ValueError(f"{who}: h must be f32 or bf16 [B, Tx] or [B, Tx, D] on the GPU, got {h.dtype} {tuple(h.shape)}")
    _durations(who, durations)
    B, Tx = h.shape[:2]
    dev = h.device
    if tuple(durations.shape) != (B, Tx) or durations.device != dev:
        raise ValueError(f"{who}: durations must be [{B}, {Tx}] on h's device, got {tuple(durations.shape)} on {durations.device}")
    if Tx > REGULATE_MAX_PHONEMES:
        raise ValueError(f"{who}: Tx = {Tx} above TT2_REGULATE_MAX_PHONEMES = {REGULATE_MAX_PHONEMES}")
    flat = h.dim() == 2
    h3 = h.unsqueeze(2) if flat else h
    if h3.shape[2] > UPSAMPLE_MAX_DIM:
        raise ValueError(f"{who}: D = {h3.shape[2]} above TT2_UPSAMPLE_MAX_DIM = {UPSAMPLE_MAX_DIM}")
    if h3.shape[2] > 1 and h3.stride(2) != 1:
        h3 = h3.contiguous()
    if max_frames is not None and not (0 <= int(max_frames) <= INT32_MAX):
        raise ValueError(f"{who}: max_frames must be in [0, 2^31 - 1], got {max_frames}")
    offset = float(offset)
    if not (0.0 <= offset < float("inf")):
        raise ValueError(f"{who}: offset must be finite and >= 0, got {offset}")
    default_delta = not torch.is_tensor(delta) and float(delta) == DEFAULT_DELTA
    if sigma is not None and not default_delta:
        raise ValueError(f"{who}: give delta or sigma, not both")
    for name, t in (("delta", delta if torch.is_tensor(delta) else None), ("sigma", sigma)):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (B, Tx) or not t.is_floating_point() or t.device != dev):
            raise ValueError(f"{who}: {name} must be a floating [{B}, {Tx}] tensor on h's device")
    lens = _lens32(who, "text_len", text_len, B, dev)
    mlen = _lens32(who, "mel_len", mel_len, B, dev)

    valid = _valid(lens, Tx, dev) if lens is not None else None
    center = centers(durations, lens).contiguous()
    bias = None
    if sigma is not None:
        s = sigma.to(torch.float32)
        if valid is not None:
            s = torch.where(valid, s, torch.ones_like(s))     # the padding's gradient is 0, not 0 * inf
        prec = (0.5 / (s * s)).contiguous()
        bias = (-torch.log(s)).contiguous()
    elif torch.is_tensor(delta):
        prec = delta.to(torch.float32).contiguous()
    else:
        prec = torch.full((B, Tx), float(delta), dtype=torch.float32, device=dev)

    if mlen is not None:
        total = mlen
    else:
        d = durations.detach()
        if valid is not None:
            d = torch.where(valid, d, torch.zeros_like(d))
        total = (d.sum(dim=1) if not d.is_floating_point() else torch.round(d.to(torch.float32).sum(dim=1))).to(torch.int64)
    if max_frames is not None:
        n_out = int(max_frames)
    else:
        n_out = int(total.max().item()) if B > 0 else 0      # the one host synchronisation
        n_out = min(max(n_out, 0), INT32_MAX)
    frames = total.clamp(0, n_out).to(torch.int32)
    y = _GaussUp.apply(h3, center, prec, bias, frames, lens, n_out, offset)
    return Upsampled(y.squeeze(2) if flat else y, frames)


class GaussianUpsampling(torch.nn.Module):
    """forward(h, durations, text_len=None, mel_len=None, max_frames=None) -> Upsampled, ESPnet's
    form with a fixed delta; see gaussian_upsample.  No parameters."""

    def __init__(self, delta: float = DEFAULT_DELTA, offset: float = 0.0):
        super().__init__()
        self.delta, self.offset = float(delta), float(offset)

    def forward(self, h, durations, text_len=None, mel_len=None, max_frames=None):
        return gaussian_upsample(h, durations, text_len=text_len, mel_len=mel_len, max_frames=max_frames,
                                 delta=self.delta, offset=self.offset)
