"""Objective scoring of decoded mels: mel-cepstral distortion after dynamic time warping (MCD-DTW).

A free-running decode has its own length and timing, so it is compared with the ground truth
along the best monotone alignment of the two sequences:

    mfcc     log-mel [B, T, 80] -> cepstra [B, T, 16] (orthonormal DCT-II, one f32 tt2_gemm)
    dtw      tt2_dtw over the cepstral columns 1..n_coef (column 0, the frame energy, is left out)
    mcd      (10 / ln 10) * sqrt(2) * total / length, in dB

and, for waveforms, by pitch along the same path (f0_metrics, f0_dtw): log-F0 RMSE in cents, gross
pitch error and voicing-decision error of the YIN tracks of tt2.audio.PitchExtractor.

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


class F0Score(NamedTuple):
    """f0_metrics(): pitch agreement of two F0 tracks along a DTW path."""
    rmse_cents: torch.Tensor     # [B] f32: RMS of 1200 log2(f_hyp / f_ref) over the doubly voiced cells (NaN: none)
    vuv_error: torch.Tensor      # [B] f32: share of the path's cells whose voicing differs (NaN: empty path)
    gpe: torch.Tensor            # [B] f32: share of the doubly voiced cells with |f_hyp / f_ref - 1| > 0.2 (NaN: none)
    voiced_pairs: torch.Tensor   # [B] int32: cells voiced on both sides


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


def f0_metrics(f0_hyp, f0_ref, path_hyp, path_ref, length) -> F0Score:
    """Pitch agreement of two F0 tracks [B, Th] and [B, Tr] (Hz, 0 = unvoiced) over the first
    length[b] cells of a DTW path (path_hyp / path_ref [B, P] frame indices, as mcd_dtw returns
    them with want_path=True).  A cell is voiced on a side when that side's f0 there is > 0.
    Sums in float64 on the tracks' device; no host synchronisation."""
    dev = f0_hyp.device
    P = path_hyp.shape[1]
    length = length.to(dev)
    live = (torch.arange(P, device=dev)[None, :] < length[:, None]) & (path_hyp >= 0) & (path_ref >= 0)
    fh = f0_hyp.to(torch.float64).gather(1, path_hyp.clamp_min(0).long())
    fr = f0_ref.to(torch.float64).gather(1, path_ref.clamp_min(0).long())
    vh, vr = (fh > 0) & live, (fr > 0) & live
    both = vh & vr
    one = torch.ones((), dtype=torch.float64, device=dev)
    ratio = torch.where(both, fh / torch.where(both, fr, one), one)
    cents = 1200.0 * torch.log2(ratio)
    n = both.sum(1).to(torch.float64)
    cells = live.sum(1).to(torch.float64)
    rmse = torch.sqrt((cents * cents).sum(1) / n)                       # 0 / 0 = NaN where nothing is voiced twice
    gpe = (((ratio - 1.0).abs() > 0.2) & both).sum(1).to(torch.float64) / n
    vuv = (vh != vr).sum(1).to(torch.float64) / cells
    return F0Score(rmse.float(), vuv.float(), gpe.float(), both.sum(1).to(torch.int32))


def f0_dtw(wav_hyp, hyp_len, wav_ref, ref_len, n_coef: int = 13, pitch=None):
    """F0 agreement of two waveform batches [B, Lh] and [B, Lr] (hyp_len / ref_len [B] samples or
    None) along the DTW alignment of their mel cepstra: mels of both sides, mcd_dtw with the path,
    YIN pitch of both sides (pitch: a tt2.audio.PitchExtractor, default parameters otherwise),
    f0_metrics.  Returns (F0Score, MCD).  At most 2048 frames per side (tt2_dtw)."""
    from .audio import PitchExtractor
    px = pitch or PitchExtractor()
    mel_h, fr_h = px.mx(wav_hyp, hyp_len)
    mel_r, fr_r = px.mx(wav_ref, ref_len)
    m = mcd_dtw(mel_h, fr_h, mel_r, fr_r, n_coef=n_coef, want_path=True)
    ph, pr = px(wav_hyp, hyp_len), px(wav_ref, ref_len)
    return f0_metrics(ph.f0, pr.f0, m.path_hyp, m.path_ref, m.length), m
