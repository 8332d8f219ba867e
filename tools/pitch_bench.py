"""Cost of YIN pitch extraction on the GPU against what one had to do before (dev tool, GPU).

Shape: B = 16 utterances of 800 frames (204544 samples each at hop 256), lags 37..339 (65..600 Hz),
threshold 0.1: 12800 frames of 512 lags x 512 samples.

* yin:        the tt2_yin launch alone on the padded buffer (f0, lag, aper, energy; no d' output);
* yin_cmnd:   the same with d'(0..tau_max) of every frame written out;
* extractor:  the whole tt2.audio.PitchExtractor call (tt2_reflect_pad, the frame counts, four
              result tensors, tt2_yin);
* torch:      the baseline on the GPU: unfold the padded buffer into frames and lagged windows, batched
              differences, squares and sums per utterance, then the running sum and d' (its d' is
              compared with tt2_yin's first);
* numpy:      tests/_yin_refs.py's float64 reference on ONE utterance, on the host.

Each GPU path is timed twice: "resident", ten back-to-back runs in a replayed hipGraph (the 13 MB
of samples stay in the caches), and "evicted", single runs between device events after a 1 GiB
buffer has been rewritten (samples come from HBM).  Rounds are interleaved.  The derived figures
(lane-operations per second, share of the VALU issue rate) come from the resident launch time and
the operation count of the definition, not from in-kernel counters.

    python tools/pitch_bench.py [--rounds 5] [--out FILE]

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

from _bench import speech_like, timed_rounds, wall_us  # noqa: E402

B, T = 16, 800
CLOCK_GHZ, SIMDS = 2.4, 1024


def torch_cmnd(padded, Lp, tau_max):
    """d'(0..tau_max) [B, T, tau_max + 1] with torch ops: one utterance at a time (its lagged
    windows are a [T, tau_max + 1, 512] view; the differences materialise 0.6 GB)."""
    frames = padded.view(B, Lp).unfold(1, 1024, 256)[:, :T]              # [B, T, 1024] view
    tau = torch.arange(tau_max + 1, device=padded.device, dtype=torch.float32)
    out = []
    for b in range(B):
        win = frames[b].unfold(1, 512, 1)[:, :tau_max + 1]                # [T, lags, 512] view
        d = ((frames[b, :, None, :512] - win) ** 2).sum(-1)
        d[:, 0] = 0
        S = torch.cumsum(d, 1)
        cm = torch.where(S > 0, d * tau / S, torch.ones_like(S))
        cm[:, 0] = 1
        out.append(cm)
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _yin_refs as R
    from tt2 import audio, ops
    dev = "cuda"
    L = (T - 1) * 256
    wav = speech_like(B, L).to(dev)
    mx = audio.MelExtractor()
    px = audio.PitchExtractor(mx)
    P = mx.plan(B, L)
    assert P.T == T
    ref = px(wav)
    padded = P.padded.clone()
    f0 = torch.empty(B, T, device=dev)
    lag = torch.empty(B, T, dtype=torch.int32, device=dev)
    aper, en = torch.empty_like(f0), torch.empty_like(f0)
    cm = torch.empty(B, T, px.tau_max + 1, device=dev)
    args = (padded, P.Lp, f0, lag, aper, en, 256, px.tau_min, px.tau_max, 22050.0, px.threshold)

    def yin():
        ops.yin(*args)

    def yin_cmnd():
        ops.yin(*args, cmnd=cm)

    def extractor():
        px(wav)

    yin_cmnd()
    torch.cuda.synchronize()
    assert torch.equal(f0.view(torch.int32), ref.f0.view(torch.int32))      # the extractor's launch, by hand
    base = torch_cmnd(padded, P.Lp, px.tau_max)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_frames = [R.yin_frame(y, px.tau_min, px.tau_max, px.threshold) for y in R.frames_of(padded[:P.Lp].cpu().numpy(), T)]
    numpy_s = time.perf_counter() - t0
    n_cm = np.stack([r["cmnd"][:px.tau_max + 1] for r in n_frames])
    k_cm = cm[0].cpu().numpy().astype(np.float64)
    n_lag = np.array([r["lag"] for r in n_frames])
    agree = {"torch_cmnd_max_rel": float(((base - cm).abs() / base).max()),
             "numpy_cmnd_max_rel_utt0": float((np.abs(k_cm - n_cm) / n_cm).max()),
             "numpy_lag_equal_utt0": float((n_lag == lag[0].cpu().numpy()).mean()),
             "voiced_share": float((f0 > 0).float().mean())}

    fns = {"yin": yin, "yin_cmnd": yin_cmnd, "extractor": extractor}
    tdp = []
    res_us, evi_us = timed_rounds(fns, a.rounds, torch.zeros(1 << 28, device=dev),
                                  each_round=lambda: tdp.append(wall_us(lambda: torch_cmnd(padded, P.Lp, px.tau_max))))
    best = {k: min(v) for k, v in res_us.items()}
    pairs = B * T * 512 * 512                       # (lag, sample) pairs: one subtract and one fma each
    lane_ops = 2 * pairs
    floor_unpacked = lane_ops / (SIMDS * 32 * CLOCK_GHZ * 1e3)   # us: 32 lanes per clock per SIMD
    res = {"shape": dict(B=B, frames=T, samples=L, tau_min=px.tau_min, tau_max=px.tau_max), "agree": agree,
           "rounds": a.rounds,
           "resident_us_best": {k: round(v, 2) for k, v in best.items()},
           "resident_us_median": {k: round(statistics.median(v), 2) for k, v in res_us.items()},
           "evicted_us_best": {k: round(min(v), 2) for k, v in evi_us.items()},
           "torch_us_best": round(min(tdp), 1), "numpy_one_utterance_us": round(numpy_s * 1e6, 1),
           "derived": {"pairs": pairs, "valu_floor_us_unpacked": round(floor_unpacked, 1),
                       "valu_floor_us_packed": round(floor_unpacked / 2, 1),
                       "lds_naive_us_one_dword_per_pair": round(pairs * 4 / (256 * 128 * CLOCK_GHZ * 1e3), 1),
                       "pairs_per_ns": round(pairs / (best["yin"] * 1e3), 1),
                       "cycles_per_frame_per_simd": round(best["yin"] * 1e3 * CLOCK_GHZ * SIMDS / (B * T), 0)},
           "speedup_vs_torch": round(min(tdp) / best["yin_cmnd"], 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
