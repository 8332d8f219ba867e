"""Cost of loudness normalisation on the GPU against what one had to do before (dev tool, GPU).

Shape: B = 16 utterances of 204544 samples at 22.05 kHz (800 mel frames: the resampler benchmark's
output), synthetic speech-like audio (pitch_bench.py's) at levels 2 dB apart, the defaults (-23 LKFS,
-1 dBFS, 100 ms steps), n_out = n_in.

* loudness:   the tt2_loudness call alone (five launches) into preallocated buffers;
* normalizer: the whole tt2.audio.LoudnessNormalizer.normalize call (lengths to int32, six fresh
              tensors, the call);
* torch:      the baseline on the GPU: the float64 impulse response of the two K-weighting sections,
              cut where it stays below 1e-12, applied by an FFT convolution in float64, then the
              sub-block sums, blocks, both gates by masks, the gain and the multiply (torchaudio is
              not needed; its gate decisions, loudness and gain are compared with tt2_loudness's
              first);
* numpy:      tests/_loudness_refs.py's float64 reference (two lfilter sections) on ONE utterance,
              on the host.

Each GPU path is timed twice: "resident", ten back-to-back runs in a replayed hipGraph (the samples
stay in the caches; the torch baseline's ten runs are eager, its FFTs are not captured), and
"evicted", single runs between device events after a 1 GiB buffer has been rewritten (samples come
from HBM).  Rounds are interleaved.  The derived figures come from the call
times and the definition's counts: bytes = 4 * (2 * sum(len) + B * n_out), each sample read by the
two filter passes and by the gain, each output column written once.

    python tools/loudness_bench.py [--rounds 5] [--out FILE]
    python tools/loudness_bench.py --calls 200          # only tt2_loudness calls, for a kernel trace

Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench import HBM_GBPS, speech_like, timed_rounds  # noqa: E402

B, N, SR = 16, 204544, 22050


def levelled_speech():
    """[B, N] f32: utterance b is 2 b dB below utterance 0."""
    return speech_like(B, N) * (10.0 ** (-2.0 * torch.arange(B) / 20.0))[:, None]


def impulse_response(coef, floor=1e-12):
    """The cascade's float64 impulse response up to the last sample at or above `floor`."""
    import _loudness_refs as R
    d = np.zeros(16384)
    d[0] = 1.0
    h = R.filter_lfilter(d, coef)
    last = int(np.nonzero(np.abs(h) >= floor)[0].max())
    assert last < len(h) - 1
    return h[:last + 1]


class TorchLoudness:
    """Measure and normalise with torch ops on the GPU; lens all equal to x.shape[1] here."""

    def __init__(self, nz, n, dev):
        self.nz = nz
        h = impulse_response(nz.coef)
        self.taps = len(h)
        self.nfft = 1 << int(np.ceil(np.log2(n + len(h))))
        self.H = torch.fft.rfft(torch.from_numpy(h).to(dev), self.nfft)

    def __call__(self, x):
        nz, n = self.nz, x.shape[1]
        y = torch.fft.irfft(torch.fft.rfft(x.double(), self.nfft) * self.H, self.nfft)[:, :n]
        S = n // nz.step
        sub = y[:, :S * nz.step].square().view(x.shape[0], S, nz.step).sum(-1)
        E = ((sub[:, :-3] + sub[:, 1:-2]) + sub[:, 2:-1]) + sub[:, 3:]
        pa = E > nz.abs_sum
        G1 = (E * pa).sum(1) / pa.sum(1).clamp_min(1)
        both = pa & (E > nz.rel_ratio * G1[:, None])
        cnt = both.sum(1)
        ms = (E * both).sum(1) / cnt.clamp_min(1) / (4.0 * nz.step)
        loud = torch.where(cnt > 0, -0.691 + 10.0 * torch.log10(ms), torch.full_like(ms, -float("inf")))
        peak = x.abs().amax(1)
        gt, ct = torch.sqrt(nz.target_ms / ms), nz.ceiling / peak.double()
        gain = torch.where(cnt > 0, torch.minimum(gt, ct), torch.ones_like(gt)).float()
        return gain[:, None] * x, loud.float(), gain, peak, ((ct < gt) & (cnt > 0)).int(), both


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=0, help="only this many tt2_loudness calls (for a kernel trace)")
    a = ap.parse_args()
    import _loudness_refs as R
    from tt2 import audio, ops
    dev = "cuda"
    nz = audio.LoudnessNormalizer()
    wav = levelled_speech().to(dev)
    lens = torch.full((B,), N, dtype=torch.int32, device=dev)
    y = torch.empty(B, N, device=dev)
    loud, gain, peak = (torch.empty(B, device=dev) for _ in range(3))
    lim = torch.empty(B, dtype=torch.int32, device=dev)
    energy = torch.empty(B, N // nz.step + 1, device=dev)
    ws = ops.Workspace()

    def loudness():
        ops.loudness(wav, nz.step, nz.coef, nz.abs_sum, nz.rel_ratio, nz.target_ms, nz.ceiling, lens=lens, y=y,
                     loud=loud, gain=gain, peak=peak, limited=lim, workspace=ws)

    def normalizer():
        nz.normalize(wav, lens)

    if a.calls:
        for _ in range(a.calls):
            loudness()
        torch.cuda.synchronize()
        return
    tl = TorchLoudness(nz, N, dev)

    def torch_base():
        return tl(wav)

    loudness()
    ops.loudness(wav, nz.step, nz.coef, nz.abs_sum, nz.rel_ratio, nz.target_ms, nz.ceiling, lens=lens, energy=energy,
                 workspace=ws)
    ty, tloud, tgain, tpeak, tlim, tboth = torch_base()
    torch.cuda.synchronize()
    p = R.default_params()
    own = [R.gate(energy[b, :N // nz.step].double().cpu().numpy(), nz.step, nz.abs_sum, nz.rel_ratio)[3] for b in range(B)]
    x0 = wav[0].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.reference(x0[None, :], None, n_out=N, **p)
    numpy_s = time.perf_counter() - t0
    t = nz.normalize(wav, lens)
    g64 = gain.double()
    agree = {"torch_same_gates": bool(all(np.array_equal(o, tboth[b].cpu().numpy()) for b, o in enumerate(own))),
             "torch_loud_max_diff": float((tloud - loud).abs().max()),
             "torch_gain_max_rel": float(((tgain.double() - g64) / g64).abs().max()),
             "torch_y_max_abs": float((ty - y).abs().max()),
             "torch_peak_limited_equal": bool(torch.equal(tpeak, peak) and torch.equal(tlim, lim)),
             "numpy_utt0": {"loud_diff": float(abs(float(loud[0]) - float(ref["loud"][0]))),
                            "gain_equal_bits": bool(float(gain[0]) == float(ref["gain"][0])),
                            "y_equal_bits": bool(np.array_equal(y[0].cpu().numpy(), ref["y"][0]))},
             "normalizer_equal_bits": bool(torch.equal(t.audio, y) and torch.equal(t.loud, loud) and torch.equal(t.gain, gain)
                                           and torch.equal(t.limited, lim)),
             "loud": [round(float(loud.min()), 3), round(float(loud.max()), 3)], "limited": int(lim.sum()),
             "blocks_passing": [int(o.sum()) for o in own][:4], "torch_taps": tl.taps, "torch_nfft": tl.nfft}
    fns = {"loudness": loudness, "normalizer": normalizer, "torch": torch_base}
    # (the FFTs are not captured: timed eagerly)
    res_us, evi_us = timed_rounds(fns, a.rounds, torch.zeros(1 << 28, device=dev), eager=("torch",), eager_runs=10)
    best = {k: min(v) for k, v in res_us.items()}
    evi = {k: min(v) for k, v in evi_us.items()}
    nbytes = 4 * (2 * int(lens.sum()) + B * N)
    floor_us = nbytes / (HBM_GBPS * 1e3)
    line = json.dumps({
        "shape": dict(B=B, samples=N, step=nz.step, target=nz.target, peak_db=nz.peak_db, n_out=N),
        "agree": agree, "rounds": a.rounds,
        "resident_us_best": {k: round(v, 2) for k, v in best.items()},
        "resident_us_median": {k: round(statistics.median(v), 2) for k, v in res_us.items()},
        "evicted_us_best": {k: round(v, 2) for k, v in evi.items()},
        "numpy_one_utterance_us": round(numpy_s * 1e6, 1),
        "derived": {"bytes": nbytes, "hbm_floor_us": round(floor_us, 2),
                    "gb_per_s_resident": round(nbytes / (best["loudness"] * 1e3), 1),
                    "gb_per_s_evicted": round(nbytes / (evi["loudness"] * 1e3), 1),
                    "x_hbm_floor_resident": round(best["loudness"] / floor_us, 1),
                    "x_hbm_floor_evicted": round(evi["loudness"] / floor_us, 1),
                    "speedup_vs_torch_resident": round(best["torch"] / best["loudness"], 1),
                    "speedup_vs_torch_evicted": round(evi["torch"] / evi["loudness"], 1)}})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
