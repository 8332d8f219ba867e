"""Objective scoring of decoded mels: mel-cepstral distortion after dynamic time warping (MCD-DTW).

A free-running decode has its own length and timing, so it is compared with the ground truth
along the best monotone alignment of the two sequences:

    mfcc     log-mel [B, T, 80] -> cepstra [B, T, 16] (orthonormal DCT-II, one f32 tt2_gemm)
    dtw      tt2_dtw over the cepstral columns 1..n_coef (column 0, the frame energy, is left out)
    mcd      (10 / ln 10) * sqrt(2) * total / length, in dB

Everything runs on the current stream without host synchronisation; results are fresh tensors
outside any arena, and the move-code scratch is this module's own, so a captured training step
stays valid.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import ops

MFCC_LD = 16   # floats per cepstral row: columns 0..n_coef, zero padding after
MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)

_WS = ops.Workspace()
_BASIS: dict = {}


class DTW(NamedTuple):
    """dtw(): the best monotone alignment of two feature sequences per utterance."""
    total: torch.Tensor    # [B] f32: accumulated frame distance along the path
    length: torch.Tensor   # [B] int32: cells on the path (0 for an empty utterance)
    path_a: torch.Tensor | None   # [B, Ta + Tb - 1] int32: row of a per path cell, -1 past length
    path_b: torch.Tensor | None   # [B, Ta + Tb - 1] int32: row of b per path cell


class MCD(NamedTuple):
    """mcd_dtw(): mel-cepstral distortion along the DTW path."""
    mcd: torch.Tensor      # [B] f32, dB (NaN where length is 0)
    total: torch.Tensor    # [B] f32
    length: torch.Tensor   # [B] int32
    path_hyp: torch.Tensor | None
    path_ref: torch.Tensor | None


def dct_basis(n_mels: int = 80, n_coef: int = 13) -> torch.Tensor:
    """Rows k = 0..n_coef of the orthonormal DCT-II over n_mels points, f32 [n_coef + 1, n_mels]
    (computed in float64 on the host): w[k][m] = s_k cos(pi (m + 1/2) k / n_mels)."""
    k = torch.arange(n_coef + 1, dtype=torch.float64)[:, None]
    m = torch.arange(n_mels, dtype=torch.float64)[None, :]
    w = torch.cos(math.pi * (m + 0.5) * k / n_mels) * math.sqrt(2.0 / n_mels)
    w[0] = math.sqrt(1.0 / n_mels)
    return w.float()


def _basis(n_mels: int, n_coef: int, dev) -> torch.Tensor:
    key = (n_mels, n_coef, str(dev))
    if key not in _BASIS:
        w = torch.zeros(MFCC_LD, n_mels, dtype=torch.float32)
        w[:n_coef + 1] = dct_basis(n_mels, n_coef)
        _BASIS[key] = w.to(dev)
    return _BASIS[key]


def mfcc(logmel: torch.Tensor, n_coef: int = 13) -> torch.Tensor:
    """Cepstra of natural-log mels [B, T, n_mels] f32: [B, T, 16] f32 with columns 0..n_coef and
    zeros after (n_coef <= 15).  One f32 tt2_gemm."""
    if not 1 <= n_coef <= MFCC_LD - 1:
        raise ValueError(f"mfcc: n_coef must be 1..{MFCC_LD - 1}")
    if logmel.dim() != 3 or logmel.dtype != torch.float32:
        raise ValueError("mfcc: log-mel must be f32 [B, T, n_mels]")
    x = logmel.contiguous()
    B, T, n_mels = x.shape
    out = torch.empty(B, T, MFCC_LD, dtype=torch.float32, device=x.device)
    if B * T:
        ops.gemm(x, _basis(n_mels, n_coef, x.device), out, B * T, MFCC_LD, n_mels, n_mels, n_mels, MFCC_LD)
    return out


def dtw(a, a_len, b, b_len, cols=None, want_path: bool = False) -> DTW:
    """tt2_dtw over feature columns cols = (c0, c1) of a [B, Ta, C] and b [B, Tb, C] f32; a_len /
    b_len [B] (or None: every row)."""
    B, ta, tb = a.shape[0], a.shape[1], b.shape[1]
    dev = a.device
    total = torch.empty(B, dtype=torch.float32, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    pa = pb = None
    if want_path:
        pa = torch.empty(B, max(0, ta + tb - 1), dtype=torch.int32, device=dev)
        pb = torch.empty_like(pa)
    al = None if a_len is None else a_len.to(dev, torch.int32).contiguous()
    bl = None if b_len is None else b_len.to(dev, torch.int32).contiguous()
    ops.dtw(a, b, total, length, a_len=al, b_len=bl, cols=cols, path_a=pa, path_b=pb, ws=_WS)
    return DTW(total, length, pa, pb)


def mcd_dtw(mel_hyp, hyp_len, mel_ref, ref_len, n_coef: int = 13, want_path: bool = False) -> MCD:
    """Mel-cepstral distortion in dB between decoded and reference natural-log mels [B, T, 80]
    along their DTW alignment, over cepstral columns 1..n_coef."""
    ch, cr = mfcc(mel_hyp, n_coef), mfcc(mel_ref, n_coef)
    r = dtw(ch, hyp_len, cr, ref_len, cols=(1, n_coef + 1), want_path=want_path)
    mcd = MCD_SCALE * r.total / r.length.float()
    mcd = torch.where(r.length > 0, mcd, torch.full_like(mcd, float("nan")))
    return MCD(mcd, r.total, r.length, r.path_a, r.path_b)
