"""Audio data path either side of the mel engine.

* ``MelExtractor``: waveform batch -> log-mel targets [B, T, 80] in the model's
  channels-last layout, Tacotron2 convention (22.05 kHz, n_fft 1024, hop 256,
  periodic Hann, centre reflect padding, magnitude, 80 Slaney mel bands over
  0..8000 Hz, log(max(x, 1e-5))).
* ``GriffinLim``: synthesised log-mels -> waveform (mel -> linear magnitude by the
  filterbank's pseudo-inverse, then Griffin-Lim with the least-squares iSTFT): the
  vocoder hand-off for listening tests.
* ``PitchExtractor``: waveform batch -> YIN F0, voicing, aperiodicity and RMS energy per
  frame of the same grid (tt2_yin on the reflect-padded buffer), and ``phoneme_average``
  for the phoneme-level pitch and energy of a duration-based student.
* ``PitchTracker``: the same, with F0 and voicing from one Viterbi path per utterance through
  the lags and an unvoiced state over YIN's d' (tt2_pitch_track) instead of a decision per frame.
* ``Resampler`` / ``resample_bank``: waveform batch at any integer rate -> 22.05 kHz (or any other
  rate) by a polyphase Kaiser-windowed sinc bank designed in float64 on the host (tt2_resample, one
  launch per batch): the step in front of everything above for corpora that ship at 24, 44.1 or
  48 kHz.
* ``SilenceTrimmer``: leading and trailing silence off a batch, by frame energy relative to the
  utterance's loudest frame (tt2_trim; librosa.effects.trim's rule), optionally behind a Resampler:
  the step that VCTK-like corpora need before alignments and stop tokens can be learnt.
* ``LoudnessNormalizer`` / ``kweighting``: integrated loudness per ITU-R BS.1770-4 of every utterance
  of a batch and one gain each to a target level under a sample-peak ceiling (tt2_loudness: the
  K-weighting recurrence as a float64 scan), optionally behind a trimmer and a resampler: the step
  that makes energies and log-mels of corpora recorded at different levels comparable.

Every transform runs on the GPU through libtt2: the window-folded DFT basis, its
inverse and the mel filterbank are f32 ``tt2_gemm`` operands (constant tables built
once at construction), and csrc/audio.hip does the padding, magnitude, phase
projection, overlap-add and log/exp row moves.  The frames of the whole batch are
one strided GEMM operand (ld = hop) over a padded buffer whose per-utterance length
is a multiple of the hop (see include/tt2_capi.h).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import ops
from ._lib import ACT_RELU, check, lib, ptr, stream_ptr

SR, N_FFT, HOP, N_MELS, FMIN, FMAX, LOG_CLAMP = 22050, 1024, 256, 80, 0.0, 8000.0, 1e-5
NB = N_FFT // 2 + 1          # 513 frequency bins
LD_SPEC = 1032               # [re 513 | im 513 | pad] columns of a spectrum row (16-B rows)
LD_MAG = 516                 # 513 magnitudes + pad


def _hz_to_mel(f: torch.Tensor) -> torch.Tensor:
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return torch.where(f >= min_log_hz, min_log_mel + torch.log(f.clamp_min(1e-12) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m: torch.Tensor) -> torch.Tensor:
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return torch.where(m >= min_log_mel, min_log_hz * torch.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr=SR, n_fft=N_FFT, n_mels=N_MELS, fmin=FMIN, fmax=FMAX) -> torch.Tensor:
    """[n_mels, n_fft/2 + 1] Slaney-normalised triangular filters (the algorithm of
    librosa.filters.mel, htk=False, norm='slaney'), float64 on the host."""
    d = torch.float64
    fft_f = torch.linspace(0, sr / 2, n_fft // 2 + 1, dtype=d)
    edges = _mel_to_hz(torch.linspace(float(_hz_to_mel(torch.tensor(fmin, dtype=d))),
                                      float(_hz_to_mel(torch.tensor(fmax, dtype=d))), n_mels + 2, dtype=d))
    fdiff = edges[1:] - edges[:-1]
    ramps = edges[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = torch.clamp(torch.minimum(lower, upper), min=0.0)
    return w * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def _window(n=N_FFT) -> torch.Tensor:
    return 0.5 - 0.5 * torch.cos(2 * math.pi * torch.arange(n, dtype=torch.float64) / n)


def n_frames(n_samples: int) -> int:
    return 1 + n_samples // HOP


class _Plan:
    """Buffers of one (batch, samples) shape."""

    def __init__(self, B: int, L: int, dev):
        self.B, self.L = B, L
        self.Lp = -(-(L + N_FFT) // HOP) * HOP          # padded length per utterance, multiple of hop
        self.R = self.Lp // HOP                          # frame rows per utterance
        self.M = B * self.R - (N_FFT // HOP - 1)         # frame rows of the batch matrix (last one in bounds)
        self.T = n_frames(L)
        f32 = dict(dtype=torch.float32, device=dev)
        self.padded = torch.zeros(B * self.Lp, **f32)
        self.spec = torch.zeros(B * self.R, LD_SPEC, **f32)
        self.mag = torch.zeros(B * self.R, LD_MAG, **f32)
        self.rows = torch.zeros(B * self.R, N_MELS, **f32)


class MelExtractor:
    def __init__(self, device="cuda"):
        self.dev = torch.device(device)
        w = _window()
        n = torch.arange(N_FFT, dtype=torch.float64)
        k = torch.arange(NB, dtype=torch.float64)
        ang = 2 * math.pi * k[:, None] * n[None, :] / N_FFT
        basis = torch.zeros(LD_SPEC, N_FFT, dtype=torch.float64)
        basis[:NB] = torch.cos(ang) * w            # Re X_k = sum_n w[n] x[n] cos(2 pi k n / N)
        basis[NB:2 * NB] = -torch.sin(ang) * w     # Im X_k = -sum_n w[n] x[n] sin(2 pi k n / N)
        self.basis = basis.float().to(self.dev)
        fb = torch.zeros(N_MELS, LD_MAG, dtype=torch.float64)
        fb[:, :NB] = mel_filterbank()
        self.fb = fb.float().to(self.dev)
        self.plans: dict[tuple[int, int], _Plan] = {}

    def plan(self, B: int, L: int) -> _Plan:
        if L <= N_FFT // 2:
            raise ValueError(f"utterances need more than {N_FFT // 2} samples (reflect padding)")
        key = (B, L)
        if key not in self.plans:
            self.plans[key] = _Plan(B, L, self.dev)
        return self.plans[key]

    def _reflect_pad(self, x: torch.Tensor, lens: torch.Tensor | None, P: _Plan):
        check(lib().tt2_reflect_pad(x.data_ptr(), x.stride(0), ptr(lens), P.B, P.L, P.padded.data_ptr(), P.Lp,
                                    N_FFT // 2, stream_ptr()), "tt2_reflect_pad")

    def _dft(self, P: _Plan):
        ops.gemm(P.padded, self.basis, P.spec, P.M, LD_SPEC, N_FFT, HOP, N_FFT, LD_SPEC)

    def stft(self, x: torch.Tensor, lens: torch.Tensor | None, P: _Plan):
        """P.spec rows [b * R + f] = [Re | Im] STFT of utterance b's frame f (f32)."""
        self._reflect_pad(x, lens, P)
        self._dft(P)

    def _padded(self, audio: torch.Tensor, lens: torch.Tensor | None):
        """Reflect-pad audio [B, L] into its plan's buffer -> (P, lens as int32 on the device or None,
        frames [B] int32 = 1 + lens // 256, or P.T without lens): the grid of the mel and pitch features."""
        B, Lx = audio.shape
        audio = audio.to(self.dev, torch.float32).contiguous()
        P = self.plan(B, Lx)
        lens32 = lens.to(self.dev, torch.int32) if lens is not None else None
        self._reflect_pad(audio, lens32, P)
        frames = (1 + lens32 // HOP) if lens32 is not None else torch.full((B,), P.T, dtype=torch.int32,
                                                                              device=self.dev)
        return P, lens32, frames

    def __call__(self, audio: torch.Tensor, lens: torch.Tensor | None = None):
        """audio [B, L] f32 (device), lens [B] samples (optional, each > 512).
        Returns (log-mel [B, T, 80] f32, frames [B] int32) with T = 1 + L // 256;
        frames past an utterance's own 1 + len // 256 hold log(1e-5) (silence)."""
        P, _, frames = self._padded(audio, lens)
        self._dft(P)
        L = lib()
        check(L.tt2_spec_magnitude(P.spec.data_ptr(), LD_SPEC, P.M, NB, P.mag.data_ptr(), LD_MAG, stream_ptr()),
              "tt2_spec_magnitude")
        ops.gemm(P.mag, self.fb, P.rows, P.M, N_MELS, LD_MAG, LD_MAG, LD_MAG, N_MELS)
        mel = torch.empty(P.B, P.T, N_MELS, dtype=torch.float32, device=self.dev)
        check(L.tt2_mel_rows(P.rows.data_ptr(), N_MELS, mel.data_ptr(), frames.data_ptr(), P.B, P.T, N_MELS, P.R,
                             LOG_CLAMP, 0, stream_ptr()), "tt2_mel_rows")
        return mel, frames


class GriffinLim:
    """log-mel [B, T, 80] -> waveform [B, (T - 1) * 256] by Griffin-Lim (zero initial phase)."""

    def __init__(self, extractor: MelExtractor | None = None, n_iter: int = 32):
        self.mx = extractor or MelExtractor()
        self.n_iter = n_iter
        dev = self.mx.dev
        w = _window()
        n = torch.arange(N_FFT, dtype=torch.float64)
        k = torch.arange(NB, dtype=torch.float64)
        ang = 2 * math.pi * n[:, None] * k[None, :] / N_FFT
        ck = torch.full((NB,), 2.0, dtype=torch.float64)
        ck[0] = ck[-1] = 1.0
        ib = torch.zeros(N_FFT, LD_SPEC, dtype=torch.float64)
        ib[:, :NB] = torch.cos(ang) * ck / N_FFT * w[:, None]        # irfft, synthesis window folded in
        ib[:, NB:2 * NB] = -torch.sin(ang) * ck / N_FFT * w[:, None]
        ib[:, NB] = 0.0
        ib[:, 2 * NB - 1] = 0.0                                     # imaginary DC / Nyquist ignored
        self.ibasis = ib.float().to(dev)
        pinv = torch.zeros(LD_MAG, N_MELS, dtype=torch.float64)
        pinv[:NB] = torch.linalg.pinv(mel_filterbank())
        self.pinv = pinv.float().to(dev)

    def __call__(self, logmel: torch.Tensor, frames: torch.Tensor | None = None):
        B, T, _ = logmel.shape
        Ls = (T - 1) * HOP
        mx = self.mx
        P = mx.plan(B, Ls)
        dev = mx.dev
        logmel = logmel.to(dev, torch.float32).contiguous()
        fr = frames.to(dev, torch.int32) if frames is not None else torch.full((B,), T, dtype=torch.int32, device=dev)
        lens = ((fr - 1) * HOP).clamp_min(N_FFT // 2 + 1).to(torch.int32)
        L = lib()
        # linear magnitude = relu(pinv(fb) exp(logmel)), in the frame-row layout
        check(L.tt2_mel_rows(P.rows.data_ptr(), N_MELS, logmel.data_ptr(), fr.data_ptr(), B, T, N_MELS, P.R,
                             LOG_CLAMP, 1, stream_ptr()), "tt2_mel_rows")
        mag = torch.zeros(B * P.R, LD_MAG, dtype=torch.float32, device=dev)
        ops.gemm(P.rows, self.pinv, mag, B * P.R, LD_MAG, N_MELS, N_MELS, N_MELS, LD_MAG, act=ACT_RELU)
        spec = torch.empty(B * P.R, LD_SPEC, dtype=torch.float32, device=dev)
        frames_td = torch.empty(B * P.R, N_FFT, dtype=torch.float32, device=dev)
        y = torch.zeros(B, Ls, dtype=torch.float32, device=dev)
        est = None
        for it in range(self.n_iter + 1):
            check(L.tt2_spec_rephase(mag.data_ptr(), LD_MAG, ptr(est), LD_SPEC, B * P.R, NB, spec.data_ptr(),
                                     LD_SPEC, stream_ptr()), "tt2_spec_rephase")
            ops.gemm(spec, self.ibasis, frames_td, B * P.R, N_FFT, LD_SPEC, LD_SPEC, LD_SPEC, N_FFT)
            check(L.tt2_overlap_add(frames_td.data_ptr(), N_FFT, lens.data_ptr(), B, Ls, P.R, N_FFT, HOP,
                                    y.data_ptr(), Ls, stream_ptr()), "tt2_overlap_add")
            if it == self.n_iter:
                break
            mx.stft(y, lens, P)
            est = P.spec
        return y, lens


class Pitch(NamedTuple):
    """PitchExtractor(): per-frame pitch features on MelExtractor's frame grid."""
    f0: torch.Tensor             # [B, T] f32, Hz; 0 where unvoiced or past the utterance
    voiced: torch.Tensor         # [B, T] bool
    aperiodicity: torch.Tensor   # [B, T] f32: d'(lag) of YIN, 1 past the utterance
    energy: torch.Tensor         # [B, T] f32: RMS of the frame's 1024 samples, 0 past the utterance
    frames: torch.Tensor         # [B] int32


class PitchExtractor:
    """YIN pitch (tt2_yin; include/tt2_capi.h has the definition) and RMS energy of every mel frame.
    Lags run from ceil(sr / fmax) to min(511, floor(sr / fmin)): at 22.05 kHz a pitch below 43.2 Hz
    is out of reach of the 1024-sample frame."""

    def __init__(self, extractor: MelExtractor | None = None, fmin: float = 65.0, fmax: float = 600.0,
                 threshold: float = 0.1):
        if not (0 < fmin <= fmax) or not threshold > 0:
            raise ValueError("PitchExtractor: 0 < fmin <= fmax and threshold > 0")
        self.mx = extractor or MelExtractor()
        self.fmin, self.fmax, self.threshold = float(fmin), float(fmax), float(threshold)
        self.tau_min = max(1, math.ceil(SR / fmax))
        self.tau_max = min(N_FFT // 2 - 1, math.floor(SR / fmin))
        if self.tau_min > self.tau_max:
            raise ValueError(f"PitchExtractor: no lag between {fmin} and {fmax} Hz fits the frame")

    def params(self) -> dict:
        return {"sr": SR, "hop": HOP, "frame": N_FFT, "fmin": self.fmin, "fmax": self.fmax,
                "threshold": self.threshold, "tau_min": self.tau_min, "tau_max": self.tau_max}

    def __call__(self, audio: torch.Tensor, lens: torch.Tensor | None = None) -> Pitch:
        """audio [B, L] f32, lens [B] samples (optional, each > 512) -> Pitch with [B, T] tensors,
        T = 1 + L // 256 and frames = 1 + lens // 256: MelExtractor's grid.  One tt2_reflect_pad
        into the extractor's plan buffer and one tt2_yin launch on the current stream; no host
        synchronisation; the results are fresh tensors."""
        f0, _, aper, energy, frames, _ = self._yin(audio, lens, False)
        return Pitch(f0, f0 > 0, aper, energy, frames)

    def _yin(self, audio, lens, want_cmnd: bool):
        """The pad and the tt2_yin launch -> (f0, lag, aper, energy, frames, cmnd or None), fresh
        tensors; cmnd [B, T, tau_max + 1] is d'(0 .. tau_max) of every valid frame (PitchTracker)."""
        P, _, frames = self.mx._padded(audio, lens)
        B, dev = P.B, self.mx.dev
        f0 = torch.empty(B, P.T, dtype=torch.float32, device=dev)
        lag = torch.empty(B, P.T, dtype=torch.int32, device=dev)
        aper, energy = torch.empty_like(f0), torch.empty_like(f0)
        cmnd = torch.empty(B, P.T, self.tau_max + 1, dtype=torch.float32, device=dev) if want_cmnd else None
        ops.yin(P.padded, P.Lp, f0, lag, aper, energy, HOP, self.tau_min, self.tau_max, SR, self.threshold,
                frames=frames, cmnd=cmnd)
        return f0, lag, aper, energy, frames, cmnd


class PitchTrack(NamedTuple):
    """PitchTracker.track(): the Pitch plus the tracked lags and the cost of each utterance's path."""
    pitch: Pitch
    lag: torch.Tensor            # [B, T] int32: the lag of a voiced frame, 0 unvoiced, -1 past the utterance
    cost: torch.Tensor           # [B] f32


class PitchTracker:
    """Viterbi pitch tracking (tt2_pitch_track; include/tt2_capi.h has the definition) over the d'
    of a PitchExtractor's tt2_yin launch: one path per utterance through the extractor's lags and
    one unvoiced state instead of a decision per frame.  A move between two lags costs `jump` per
    octave (pos = log2 of the lag), a change of voicing costs `switch`, and an unvoiced frame costs
    `unvoiced` where a voiced one costs its d'.  The three defaults were chosen on synthetic signals
    only.  A drop-in for PitchExtractor wherever a Pitch is wanted (data.extract_pitch,
    evaluate.f0_dtw)."""

    def __init__(self, extractor: PitchExtractor | None = None, jump: float = 1.0, switch: float = 0.1,
                 unvoiced: float = 0.2):
        for name, v in (("jump", jump), ("switch", switch), ("unvoiced", unvoiced)):
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"PitchTracker: {name} must be finite and not negative")
        self.px = extractor or PitchExtractor()
        self.jump, self.switch, self.unvoiced = float(jump), float(switch), float(unvoiced)
        self._pos = None

    mx = property(lambda self: self.px.mx)
    tau_min = property(lambda self: self.px.tau_min)
    tau_max = property(lambda self: self.px.tau_max)

    def params(self) -> dict:
        return {**self.px.params(), "track": "viterbi", "jump": self.jump, "switch": self.switch,
                "unvoiced": self.unvoiced}

    def pos(self) -> torch.Tensor:
        """log2(tau) for tau = 0 .. tau_max (entry 0 is 0 and never read): float64 on the host,
        rounded to f32."""
        if self._pos is None:
            tau = torch.arange(self.tau_max + 1, dtype=torch.float64).clamp_min(1.0)
            self._pos = torch.log2(tau).float().to(self.mx.dev)
        return self._pos

    def track(self, audio: torch.Tensor, lens: torch.Tensor | None = None) -> PitchTrack:
        """audio [B, L] f32, lens [B] samples (optional, each > 512), as PitchExtractor takes them.
        One pad, one tt2_yin launch that also writes d' into a fresh tensor, one tt2_pitch_track
        launch; no host synchronisation.  f0 and voiced are the tracker's; aperiodicity, energy and
        frames are tt2_yin's, the bits PitchExtractor returns."""
        _, lag, aper, energy, frames, cmnd = self.px._yin(audio, lens, True)
        f0 = torch.empty_like(aper)
        cost = torch.empty(aper.shape[0], dtype=torch.float32, device=aper.device)
        ops.pitch_track(cmnd, frames, f0, lag, cost, self.tau_min, self.tau_max, SR, self.pos(), self.jump,
                        self.switch, self.unvoiced)
        return PitchTrack(Pitch(f0, lag > 0, aper, energy, frames), lag, cost)

    def __call__(self, audio: torch.Tensor, lens: torch.Tensor | None = None) -> Pitch:
        return self.track(audio, lens).pitch


class ResampleBank(NamedTuple):
    """resample_bank(): the polyphase filter bank of one rate pair."""
    up: int
    down: int
    half: int
    taps: torch.Tensor           # [up, 2 * half + 1] float64, host


def resample_bank(sr_in: int, sr_out: int, zeros: int = 24, rolloff: float = 0.9, beta: float = 10.0) -> ResampleBank:
    """The Kaiser-windowed sinc bank of tt2_resample for sr_in -> sr_out (include/tt2_capi.h has
    the definition): up = sr_out / g, down = sr_in / g, cutoff c = rolloff * min(1, up / down) of
    the input Nyquist, `zeros` zero crossings either side, half = ceil(zeros / c) taps either side.
    Row r holds h(k - f_r), k = -half .. half, f_r = ((r * down) mod up) / up.  float64 on the
    host, no device work.  The defaults (24 zeros, rolloff 0.9, beta 10) keep a tone below 0.726 of
    the lower Nyquist within 6e-6 and one above 1.15 of the new Nyquist below -105 dB."""
    from ._lib import RESAMPLE_MAX_PHASES, RESAMPLE_MAX_TAPS
    if int(sr_in) != sr_in or int(sr_out) != sr_out or sr_in < 1 or sr_out < 1:
        raise ValueError(f"resample_bank: rates must be positive integers, got {sr_in} -> {sr_out}")
    if int(zeros) != zeros or zeros < 1:
        raise ValueError(f"resample_bank: zeros must be an integer >= 1, got {zeros}")
    if not (0.0 < rolloff <= 1.0):
        raise ValueError(f"resample_bank: rolloff must be in (0, 1], got {rolloff}")
    if not (math.isfinite(beta) and beta >= 0.0):
        raise ValueError(f"resample_bank: beta must be finite and not negative, got {beta}")
    sr_in, sr_out, zeros = int(sr_in), int(sr_out), int(zeros)
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    c = float(rolloff) * min(1.0, up / down)
    half = math.ceil(zeros / c)
    if up > RESAMPLE_MAX_PHASES:
        raise ValueError(f"resample_bank: {sr_in} -> {sr_out} needs {up} phases, above "
                         f"TT2_RESAMPLE_MAX_PHASES = {RESAMPLE_MAX_PHASES}")
    if 2 * half + 1 > RESAMPLE_MAX_TAPS:
        raise ValueError(f"resample_bank: {sr_in} -> {sr_out} with {zeros} zeros needs {2 * half + 1} taps, above "
                         f"TT2_RESAMPLE_MAX_TAPS = {RESAMPLE_MAX_TAPS}")
    d = torch.float64
    r = torch.arange(up, dtype=torch.int64)
    f = ((r * down) % up).to(d) / up
    t = torch.arange(-half, half + 1, dtype=d)[None, :] - f[:, None]     # [up, K], input samples
    u = c * t / zeros
    inside = u.abs() < 1.0
    w = torch.special.i0(beta * torch.sqrt((1.0 - u * u).clamp_min(0.0))) / torch.special.i0(torch.tensor(beta, dtype=d))
    taps = c * torch.sinc(c * t) * torch.where(inside, w, torch.zeros((), dtype=d))
    return ResampleBank(up, down, half, taps)


class _Stage:
    """What the waveform stages (Resampler, SilenceTrimmer, LoudnessNormalizer) do to their input."""
    resampler = None             # the stage run first: anything of the resampler protocol

    def _prepare(self, audio, lens):
        """The front stage's output (or the input) as the kernels take it: audio f32 on the device with
        a contiguous last dim (row views stay views), lens a contiguous int32 [B] or None."""
        if self.resampler is not None:
            audio, lens = self.resampler(audio, lens)
        audio = audio.to(self.dev, torch.float32)
        if audio.stride(1) != 1 and audio.shape[1] > 1:
            audio = audio.contiguous()
        lens32 = lens.to(self.dev, torch.int32).contiguous() if lens is not None else None
        return audio, lens32


class _Chained(_Stage):
    """A stage that works at one rate `sr` and may run another (resampler=) in front of itself, so that
    one object takes a batch from the corpus's rate to this stage's output.  A subclass calls _chain
    from its constructor and gives its own parameters in _params."""

    def _chain(self, resampler, sr, device):
        if resampler is not None and int(resampler.sr_out) != int(sr):
            raise ValueError(f"{type(self).__name__}: the resampler writes {resampler.sr_out} Hz, "
                             f"this stage works at {sr} Hz")
        self.sr, self.resampler, self.dev = int(sr), resampler, torch.device(device)
        self._ws = ops.Workspace()

    sr_in = property(lambda self: self.resampler.sr_in if self.resampler is not None else self.sr)
    sr_out = property(lambda self: self.sr)

    def params(self) -> dict:
        p = self._params()
        if self.resampler is not None:
            p["resampler"] = self.resampler.params()
        return p


class Resampler(_Stage):
    """Sample-rate conversion sr_in -> sr_out (tt2_resample; include/tt2_capi.h has the definition)
    of a padded batch, with the bank of resample_bank rounded once to f32.  The corpus tool
    (tools/resample_corpus.py) and data.collate(resampler=) run it; MelExtractor, PitchExtractor
    and everything after them stay at 22.05 kHz."""

    def __init__(self, sr_in: int, sr_out: int = SR, device="cuda", zeros: int = 24, rolloff: float = 0.9,
                 beta: float = 10.0):
        self.bank = resample_bank(sr_in, sr_out, zeros, rolloff, beta)
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.zeros, self.rolloff, self.beta = int(zeros), float(rolloff), float(beta)
        self.dev = torch.device(device)
        self._taps = None

    up = property(lambda self: self.bank.up)
    down = property(lambda self: self.bank.down)
    half = property(lambda self: self.bank.half)

    def params(self) -> dict:
        return {"sr_in": self.sr_in, "sr_out": self.sr_out, "up": self.up, "down": self.down, "half": self.half,
                "zeros": self.zeros, "rolloff": self.rolloff, "beta": self.beta}

    def taps(self) -> torch.Tensor:
        """The bank on the device, [up, 2 * half + 1] f32 (uploaded on first use)."""
        if self._taps is None:
            self._taps = self.bank.taps.float().to(self.dev)
        return self._taps

    def out_len(self, n: int) -> int:
        return -(-int(n) * self.up // self.down)

    def __call__(self, audio: torch.Tensor, lens: torch.Tensor | None = None):
        """audio [B, L] f32, lens [B] samples (optional) -> (audio_out [B, ceil(L * up / down)] f32,
        out_lens [B] int32 = ceil(lens * up / down)); samples past an utterance's out_len are 0.
        One tt2_resample launch on the current stream into fresh tensors; no host synchronisation.
        With sr_in == sr_out the inputs are returned as they are (lens as an int32 tensor of L when
        None) and nothing is launched."""
        B, L = audio.shape
        if self.up == self.down:
            if lens is None:
                lens = torch.full((B,), L, dtype=torch.int32, device=audio.device)
            return audio, lens
        audio, lens32 = self._prepare(audio, lens)
        n_out = self.out_len(L)
        if B == 0 or n_out == 0:
            return (torch.zeros(B, n_out, dtype=torch.float32, device=self.dev),
                    torch.zeros(B, dtype=torch.int32, device=self.dev))
        y = torch.empty(B, n_out, dtype=torch.float32, device=self.dev)
        out_lens = torch.empty(B, dtype=torch.int32, device=self.dev)
        ops.resample(audio, y, self.taps(), self.up, self.down, self.half, lens=lens32, out_lens=out_lens)
        return y, out_lens


class Trimmed(NamedTuple):
    """SilenceTrimmer.trim(): audio [B, L] f32 (zeros past lens), lens [B] int32 samples kept, start [B]
    int32 first kept sample of the input, energy [B, L // hop + 1] f32 frame energies or None."""
    audio: torch.Tensor
    lens: torch.Tensor
    start: torch.Tensor
    energy: torch.Tensor | None


class SilenceTrimmer(_Chained):
    """Leading / trailing silence trimming of a padded batch (tt2_trim; include/tt2_capi.h has the
    definition): everything before the first and after the last frame whose energy is within top_db
    of the utterance's loudest frame goes, `keep` samples either side stay, interior silence stays.
    With keep = 0 this is librosa.effects.trim's rule with ref = np.max, and the defaults (60 dB,
    frames of 2048 at hop 512) are librosa's: they were chosen without a speech corpus, and
    validating top_db on VCTK or LibriTTS is open.  `frame` must be an even multiple of `hop`, at
    most 2 * TT2_TRIM_MAX_R hops.  With resampler=rs (a Resampler whose sr_out is `sr`) a call runs rs
    first and trims its output, so that one object takes a corpus from its own rate to trimmed
    22.05 kHz audio wherever a resampler is accepted (data.collate, data.resample_corpus,
    data.trim_corpus)."""

    def __init__(self, top_db: float = 60.0, frame: int = 2048, hop: int = 512, keep: int = 0, sr: int = SR,
                 resampler=None, device="cuda"):
        from ._lib import TRIM_MAX_R
        top_db = float(top_db)
        if not (math.isfinite(top_db) and top_db >= 0.0):
            raise ValueError(f"SilenceTrimmer: top_db must be finite and not negative, got {top_db}")
        if int(frame) != frame or int(hop) != hop or hop < 1 or frame < 2 * hop or frame % (2 * hop) \
                or frame // (2 * hop) > TRIM_MAX_R:
            raise ValueError(f"SilenceTrimmer: frame must be 2 * r * hop with 1 <= r <= TT2_TRIM_MAX_R = {TRIM_MAX_R}, "
                             f"got frame {frame}, hop {hop}")
        if int(keep) != keep or keep < 0:
            raise ValueError(f"SilenceTrimmer: keep must be an integer >= 0, got {keep}")
        self._chain(resampler, sr, device)
        self.top_db, self.frame, self.hop, self.keep = top_db, int(frame), int(hop), int(keep)
        self.r = self.frame // (2 * self.hop)
        # the power ratio in float64, rounded once to f32 (the C argument is an f32)
        self.ratio = float(torch.tensor(10.0 ** (-top_db / 10.0), dtype=torch.float64).float())

    def _params(self) -> dict:
        return {"top_db": self.top_db, "frame": self.frame, "hop": self.hop, "r": self.r, "keep": self.keep,
                "ratio": self.ratio, "sr": self.sr}

    def trim(self, audio: torch.Tensor, lens: torch.Tensor | None = None, want_energy: bool = False) -> Trimmed:
        """audio [B, L] f32 at sr_in, lens [B] samples (optional) -> Trimmed, every field a fresh
        tensor; the scratch is this object's own, grown on demand.  On the current stream, no host
        synchronisation."""
        audio, lens32 = self._prepare(audio, lens)
        B, L = audio.shape
        energy = torch.zeros(B, L // self.hop + 1, dtype=torch.float32, device=self.dev) if want_energy else None
        if B == 0 or L == 0:
            z = torch.zeros(B, dtype=torch.int32, device=self.dev)
            return Trimmed(torch.zeros(B, L, dtype=torch.float32, device=self.dev), z, z.clone(), energy)
        y = torch.empty(B, L, dtype=torch.float32, device=self.dev)
        out_lens = torch.empty(B, dtype=torch.int32, device=self.dev)
        start = torch.empty(B, dtype=torch.int32, device=self.dev)
        ops.trim(audio, y, self.hop, self.r, self.keep, self.ratio, lens=lens32, out_lens=out_lens, start=start,
                 energy=energy, workspace=self._ws)
        return Trimmed(y, out_lens, start, energy)

    def __call__(self, audio: torch.Tensor, lens: torch.Tensor | None = None):
        """(audio_out [B, L] f32, out_lens [B] int32): the resampler protocol."""
        t = self.trim(audio, lens)
        return t.audio, t.lens


def kweighting(sr: int):
    """The two K-weighting biquads of ITU-R BS.1770 at the rate sr, ((b, a), (b, a)) as tuples of three
    floats each (a[0] = 1): the high shelf, then the high-pass, from the analogue prototypes by the
    bilinear transform (the formulas of libebur128 and pyloudnorm).  At 48 kHz they are the
    standard's own table to 1e-15.  float64 on the host, no device work."""
    if int(sr) != sr or sr < 1:
        raise ValueError(f"kweighting: the rate must be a positive integer, got {sr}")
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = (((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0),
             (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0))
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    highpass = ((1.0, -2.0, 1.0), (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0))
    return shelf, highpass


class Loudness(NamedTuple):
    """LoudnessNormalizer.measure(): loud [B] f32 LKFS (-inf: unmeasured), peak [B] f32 max |x|, energy
    [B, L // step + 1] f32 sums of the squared K-weighted signal per 100 ms."""
    loud: torch.Tensor
    peak: torch.Tensor
    energy: torch.Tensor


class Normalized(NamedTuple):
    """LoudnessNormalizer.normalize(): audio [B, L] f32 (zeros past lens), lens [B] int32, loud [B] f32
    LKFS of the input, gain [B] f32 (a factor), peak [B] f32 of the input, limited [B] int32 (1: the
    peak ceiling set the gain)."""
    audio: torch.Tensor
    lens: torch.Tensor
    loud: torch.Tensor
    gain: torch.Tensor
    peak: torch.Tensor
    limited: torch.Tensor


class LoudnessNormalizer(_Chained):
    """Loudness normalisation of a padded batch (tt2_loudness; include/tt2_capi.h has the definition):
    integrated loudness per ITU-R BS.1770-4 (K-weighting, 400 ms blocks every 100 ms, the -70 LKFS
    absolute and the -10 LU relative gate), one gain per utterance that brings it to `target` LKFS
    unless the sample peak would then pass `peak_db` dBFS, in which case the peak sets the gain
    (limited).  An utterance with no block above the gates (shorter than 400 ms, silence) is
    unmeasured and passes unchanged.  No limiter, no true-peak measurement.  The defaults (-23 LUFS,
    -1 dBFS) are EBU R128's: they were chosen without a speech corpus.  With resampler=rs (any object
    of the resampler protocol whose sr_out is `sr`, a SilenceTrimmer over a Resampler for one) a call
    runs rs first, so one object takes a corpus from its own rate to trimmed, levelled audio wherever
    a resampler is accepted (data.collate, data.resample_corpus, data.normalize_corpus)."""

    def __init__(self, target: float = -23.0, peak_db: float = -1.0, sr: int = SR, resampler=None, device="cuda"):
        target, peak_db = float(target), float(peak_db)
        if not (math.isfinite(target) and math.isfinite(peak_db)):
            raise ValueError(f"LoudnessNormalizer: target and peak_db must be finite, got {target}, {peak_db}")
        if int(sr) != sr or sr < 10 or sr % 10:
            raise ValueError(f"LoudnessNormalizer: the rate must be a positive multiple of 10 (100 ms steps), got {sr}")
        self._chain(resampler, sr, device)
        self.target, self.peak_db = target, peak_db
        self.step = self.sr // 10
        (b1, a1), (b2, a2) = kweighting(self.sr)
        self.coef = (*b1, a1[1], a1[2], *b2, a2[1], a2[2])
        self.abs_sum = 4.0 * self.step * 10.0 ** ((-70.0 + 0.691) / 10.0)
        self.rel_ratio = 0.1
        self.target_ms = 10.0 ** ((target + 0.691) / 10.0)
        # the amplitude ratio in float64, rounded once to f32 (the C argument is an f32)
        self.ceiling = float(torch.tensor(10.0 ** (peak_db / 20.0), dtype=torch.float64).float())

    def _params(self) -> dict:
        return {"target": self.target, "peak_db": self.peak_db, "sr": self.sr, "step": self.step,
                "coef": list(self.coef), "abs_sum": self.abs_sum, "rel_ratio": self.rel_ratio,
                "target_ms": self.target_ms, "ceiling": self.ceiling}

    def _run(self, audio, lens32, **out):
        ops.loudness(audio, self.step, self.coef, self.abs_sum, self.rel_ratio, self.target_ms, self.ceiling,
                     lens=lens32, workspace=self._ws, **out)

    def measure(self, audio: torch.Tensor, lens: torch.Tensor | None = None) -> Loudness:
        """audio [B, L] f32 at sr_in, lens [B] samples (optional) -> Loudness, fresh tensors; no audio
        is written.  On the current stream, no host synchronisation."""
        audio, lens32 = self._prepare(audio, lens)
        B, L = audio.shape
        f = dict(dtype=torch.float32, device=self.dev)
        if B == 0 or L == 0:
            return Loudness(torch.full((B,), -math.inf, **f), torch.zeros(B, **f), torch.zeros(B, L // self.step + 1, **f))
        loud, peak = torch.empty(B, **f), torch.empty(B, **f)
        energy = torch.empty(B, L // self.step + 1, **f)
        self._run(audio, lens32, loud=loud, peak=peak, energy=energy)
        return Loudness(loud, peak, energy)

    def normalize(self, audio: torch.Tensor, lens: torch.Tensor | None = None) -> Normalized:
        """audio [B, L] f32 at sr_in, lens [B] samples (optional) -> Normalized, every field a fresh
        tensor; the scratch is this object's own, grown on demand.  On the current stream, no host
        synchronisation."""
        audio, lens32 = self._prepare(audio, lens)
        B, L = audio.shape
        f = dict(dtype=torch.float32, device=self.dev)
        out_lens = (lens32.clamp(0, L) if lens32 is not None
                    else torch.full((B,), L, dtype=torch.int32, device=self.dev))
        if B == 0 or L == 0:
            return Normalized(torch.zeros(B, L, **f), out_lens, torch.full((B,), -math.inf, **f), torch.ones(B, **f),
                              torch.zeros(B, **f), torch.zeros(B, dtype=torch.int32, device=self.dev))
        y = torch.empty(B, L, **f)
        loud, gain, peak = torch.empty(B, **f), torch.empty(B, **f), torch.empty(B, **f)
        limited = torch.empty(B, dtype=torch.int32, device=self.dev)
        self._run(audio, lens32, y=y, loud=loud, gain=gain, peak=peak, limited=limited)
        return Normalized(y, out_lens, loud, gain, peak, limited)

    def __call__(self, audio: torch.Tensor, lens: torch.Tensor | None = None):
        """(audio_out [B, L] f32, lens [B] int32): the resampler protocol."""
        n = self.normalize(audio, lens)
        return n.audio, n.lens


def phoneme_average(values: torch.Tensor, durations: torch.Tensor, mask: torch.Tensor | None = None) -> torch.Tensor:
    """Mean of values [B, T] over each phoneme's run of frames (phoneme p of utterance b owns the
    durations[b, p] frames after those of the phonemes before it), over the frames where mask
    [B, T] is true (default: all); 0 where a phoneme has no such frame.  Frames past the sum of
    the durations belong to no phoneme.  [B, Tx] in values' dtype, on values' device; cumulative
    sums in float64, no loop over frames (FastSpeech 2's phoneme-level pitch and energy)."""
    if values.dim() != 2 or durations.dim() != 2 or values.shape[0] != durations.shape[0]:
        raise ValueError("phoneme_average: values [B, T] and durations [B, Tx]")
    B, T = values.shape
    dev = values.device
    m = torch.ones(B, T, dtype=torch.float64, device=dev) if mask is None else mask.to(dev, torch.float64)
    v = torch.where(m > 0, values.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))
    zero = torch.zeros(B, 1, dtype=torch.float64, device=dev)
    cs = torch.cat([zero, v.cumsum(1)], 1)          # [B, T + 1]: sums of the frames before each index
    cn = torch.cat([zero, m.cumsum(1)], 1)
    end = durations.to(dev, torch.long).clamp_min(0).cumsum(1).clamp(max=T)
    start = torch.cat([torch.zeros(B, 1, dtype=torch.long, device=dev), end[:, :-1]], 1)
    tot = cs.gather(1, end) - cs.gather(1, start)
    cnt = cn.gather(1, end) - cn.gather(1, start)
    out = torch.where(cnt > 0, tot / cnt.clamp_min(1.0), torch.zeros_like(tot))
    return out.to(values.dtype)
