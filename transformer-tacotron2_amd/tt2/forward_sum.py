"""Forward-sum alignment loss: learn the (frame, phoneme) alignment without a teacher.

The three steps of RAD-TTS / FastPitch 1.1 / JETS over the kernels of csrc/forward_sum.hip
(include/tt2_capi.h has the definition): a small aligner scores every (frame, phoneme) pair, the
forward-sum loss maximises the total probability of all monotone alignments (CTC over the phoneme
sequence without a useful blank; Badlani et al. 2021), and a Viterbi pass over the same scores
binarises the soft alignment into durations.

* ``forward_sum_loss(scores, text_len, mel_len, reduction)``: ``-ln Z`` per utterance, differentiable
  in ``scores`` (forward tt2_forward_sum_fwd, backward tt2_forward_sum_bwd).
* ``posterior(scores, text_len, mel_len)``: the loss and ``gamma[b, n, t] = P(pi(n) = t)``.
* ``best_path(scores, text_len, mel_len)``: durations, path and mean log-probability of the best
  path, in the shapes and conventions of ``MonotonicAlignment``: ``durations`` goes into
  ``regulate.plan`` and ``path`` is that plan's ``index``.
* ``ForwardSumLoss``: the nn.Module over ``forward_sum_loss``.
* ``beta_binomial_prior``: the RAD-TTS log prior to add to the scores (pure torch).

Scores are f32 ``[B, Ty, Tx]`` or ``[B, 1, Ty, Tx]`` (frames by phonemes); the log-softmax over each
utterance's own phonemes is fused.  Nothing synchronises with the host, every result is a fresh
tensor, and all results are bit-identical run to run.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops
from ._lib import FSUM_MAX_FRAMES, FSUM_MAX_KEYS


class ForwardSum(NamedTuple):
    """posterior(): loss [B] f32 = -ln Z, gamma [B, Ty, Tx] f32 (rows sum to 1; 0 in the padding)."""
    loss: torch.Tensor
    gamma: torch.Tensor


class HardAlignment(NamedTuple):
    """best_path(): durations [B, Tx] int32, path [B, Ty] int32 (-1 past the utterance), logp [B] f32."""
    durations: torch.Tensor
    path: torch.Tensor
    logp: torch.Tensor


def _scores3(who, scores):
    if scores.dim() == 4 and scores.shape[1] == 1:
        scores = scores[:, 0]
    if scores.dim() != 3 or scores.dtype != torch.float32:
        raise ValueError(f"{who}: scores must be f32 [B, Ty, Tx] or [B, 1, Ty, Tx], got {scores.dtype} {tuple(scores.shape)}")
    if not scores.is_cuda:
        raise ValueError(f"{who}: scores must be on the GPU")
    if scores.shape[1] > FSUM_MAX_FRAMES or scores.shape[2] > FSUM_MAX_KEYS:
        raise ValueError(f"{who}: [Ty, Tx] = {tuple(scores.shape[1:])} above [{FSUM_MAX_FRAMES}, {FSUM_MAX_KEYS}]")
    if scores.shape[2] > 1 and scores.stride(2) != 1:
        scores = scores.contiguous()
    return scores


def _lens32(who, name, lens, B, dev):
    if lens is None:
        return None
    if lens.dim() != 1 or lens.shape[0] != B or lens.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: {name} must be an integer [{B}], got {lens.dtype} {tuple(lens.shape)}")
    return lens.to(device=dev, dtype=torch.int32).contiguous()


class _ForwardSum(torch.autograd.Function):
    """loss = -ln Z: forward tt2_forward_sum_fwd, backward tt2_forward_sum_bwd."""

    @staticmethod
    def forward(ctx, scores, text_len, mel_len):
        B, Ty, Tx = scores.shape
        dev = scores.device
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        lse = torch.empty(B, Ty, dtype=torch.float32, device=dev)
        alpha = torch.empty(B, Ty, Tx, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        ops.forward_sum_fwd(scores, loss, lse, alpha, q_len=mel_len, key_len=text_len)
        if alpha is not None:
            ctx.save_for_backward(scores, lse, alpha, text_len, mel_len)
        return loss

    @staticmethod
    def backward(ctx, grad):
        scores, lse, alpha, text_len, mel_len = ctx.saved_tensors
        dscores = torch.empty(scores.shape, dtype=torch.float32, device=scores.device)
        grad = grad.to(torch.float32).contiguous()      # a gradient can arrive expanded (stride 0)
        ops.forward_sum_bwd(scores, lse, alpha, dscores=dscores, grad_loss=grad, q_len=mel_len, key_len=text_len)
        return dscores, None, None


def forward_sum_loss(scores: torch.Tensor, text_len: torch.Tensor | None = None, mel_len: torch.Tensor | None = None,
                     reduction: str = "mean") -> torch.Tensor:
    """scores [B, Ty, Tx] or [B, 1, Ty, Tx] f32 on the GPU, text_len [B] (phonemes per utterance; None:
    Tx), mel_len [B] (frames; None: Ty) -> the forward-sum loss.  reduction "none": -ln Z per
    utterance [B]; "sum": their sum; "mean": sum_b loss_b / max(Tx_b, 1) / B, the convention of the
    NVIDIA and ESPnet implementations.  Differentiable in scores; the incoming gradient goes to the
    kernel as a device vector.  No host synchronisation."""
    who = "forward_sum_loss"
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"{who}: reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
    s = _scores3(who, scores)
    B, Ty, Tx = s.shape
    tl = _lens32(who, "text_len", text_len, B, s.device)
    ml = _lens32(who, "mel_len", mel_len, B, s.device)
    loss = _ForwardSum.apply(s, tl, ml)
    if reduction == "none":
        return loss
    if reduction == "sum":
        return loss.sum()
    if B == 0:
        return loss.sum()
    tx = torch.full((B,), Tx, dtype=torch.int32, device=s.device) if tl is None else tl.clamp(0, Tx)
    return (loss / tx.clamp(min=1).to(torch.float32)).sum() / B


def posterior(scores: torch.Tensor, text_len: torch.Tensor | None = None,
              mel_len: torch.Tensor | None = None) -> ForwardSum:
    """scores as in forward_sum_loss -> ForwardSum(loss [B], gamma [B, Ty, Tx]): the probability that
    frame n is on phoneme t over all monotone alignments.  Not differentiable.  No host
    synchronisation."""
    who = "posterior"
    s = _scores3(who, scores).detach()
    B, Ty, Tx = s.shape
    tl = _lens32(who, "text_len", text_len, B, s.device)
    ml = _lens32(who, "mel_len", mel_len, B, s.device)
    loss = torch.empty(B, dtype=torch.float32, device=s.device)
    lse = torch.empty(B, Ty, dtype=torch.float32, device=s.device)
    alpha = torch.empty(B, Ty, Tx, dtype=torch.float32, device=s.device)
    gamma = torch.empty(B, Ty, Tx, dtype=torch.float32, device=s.device)
    ops.forward_sum_fwd(s, loss, lse, alpha, q_len=ml, key_len=tl)
    ops.forward_sum_bwd(s, lse, alpha, gamma=gamma, q_len=ml, key_len=tl)
    return ForwardSum(loss, gamma)


def best_path(scores: torch.Tensor, text_len: torch.Tensor | None = None,
              mel_len: torch.Tensor | None = None) -> HardAlignment:
    """scores as in forward_sum_loss -> HardAlignment(durations [B, Tx] int32, path [B, Ty] int32,
    logp [B] f32): the monotone path of greatest total score (strict compare: a tie stays on the
    phoneme), the frames it gives each phoneme and the mean log-softmax along it.  No host
    synchronisation."""
    who = "best_path"
    s = _scores3(who, scores).detach()
    B, Ty, Tx = s.shape
    tl = _lens32(who, "text_len", text_len, B, s.device)
    ml = _lens32(who, "mel_len", mel_len, B, s.device)
    path = torch.empty(B, Ty, dtype=torch.int32, device=s.device)
    durations = torch.empty(B, Tx, dtype=torch.int32, device=s.device)
    logp = torch.empty(B, dtype=torch.float32, device=s.device)
    ops.forward_sum_path(s, path, durations, logp, q_len=ml, key_len=tl)
    return HardAlignment(durations, path, logp)


class ForwardSumLoss(torch.nn.Module):
    """forward(scores, text_len=None, mel_len=None) -> forward_sum_loss with the module's reduction.
    No parameters."""

    def __init__(self, reduction: str = "mean"):
        super().__init__()
        if reduction not in ("none", "sum", "mean"):
            raise ValueError(f"ForwardSumLoss: reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
        self.reduction = reduction

    def forward(self, scores, text_len=None, mel_len=None):
        return forward_sum_loss(scores, text_len, mel_len, reduction=self.reduction)


def beta_binomial_prior(text_len: torch.Tensor, mel_len: torch.Tensor, tx: int, ty: int,
                        scaling: float = 1.0) -> torch.Tensor:
    """The RAD-TTS alignment prior as a log prior [B, ty, tx] f32 to add to the scores: frame n of an
    utterance of Ty_b frames and Tx_b phonemes gets betabinom(N = Tx_b, a = w (n + 1),
    b = w (Ty_b - n)).logpmf(t) for t < Tx_b with w = scaling, and 0 in padded cells (n >= Ty_b or
    t >= Tx_b).  The support's last point t = Tx_b is dropped, as RAD-TTS does: the loss renormalises
    the row.  Pure torch (lgamma in float64), on text_len's device."""
    if text_len.dim() != 1 or mel_len.shape != text_len.shape:
        raise ValueError("beta_binomial_prior: text_len and mel_len must be [B]")
    if not scaling > 0.0:
        raise ValueError(f"beta_binomial_prior: scaling must be > 0, got {scaling}")
    dev = text_len.device
    N = text_len.to(torch.float64).clamp(0, tx)[:, None, None]
    Ty = mel_len.to(device=dev, dtype=torch.float64).clamp(0, ty)[:, None, None]
    n = torch.arange(ty, dtype=torch.float64, device=dev)[None, :, None]
    k = torch.arange(tx, dtype=torch.float64, device=dev)[None, None, :]
    valid = (n < Ty) & (k < N)
    a = torch.where(valid, float(scaling) * (n + 1.0), torch.ones_like(n))
    b = torch.where(valid, float(scaling) * (Ty - n), torch.ones_like(n))
    Nv = torch.where(valid, N, torch.ones_like(N))
    kv = torch.where(valid, k, torch.zeros_like(k))
    lg = torch.lgamma
    logpmf = (lg(Nv + 1.0) - lg(kv + 1.0) - lg(Nv - kv + 1.0)
              + lg(kv + a) + lg(Nv - kv + b) - lg(Nv + a + b)
              - (lg(a) + lg(b) - lg(a + b)))
    return torch.where(valid, logpmf, torch.zeros_like(logpmf)).to(torch.float32)
