"""Cost of sample-rate conversion on the GPU against what one had to do before (dev tool, GPU).

Shape: B = 16 utterances whose output is 204544 samples (800 mel frames), for 48000 -> 22050
(up 147, down 320, 119 taps) and 44100 -> 22050 (up 1, down 2, 109 taps), the default bank.

* resample:   the tt2_resample launch alone into preallocated buffers;
* resampler:  the whole tt2.audio.Resampler call (lengths to int32, two fresh tensors, the launch);
* torch:      the baseline on the GPU, the formulation torchaudio uses: F.conv1d at stride `down`
              over the zero-padded batch with the bank scattered into an [up, 1, 2 * half + down]
              weight, then the [B, up, periods] result transposed into samples (its values are
              compared with tt2_resample's first);
* numpy:      tests/_resample_refs.py's float64 reference on ONE utterance, on the host.

Each GPU path is timed twice: "resident", ten back-to-back runs in a replayed hipGraph (the samples
stay in the caches), and "evicted", single runs between device events after a 1 GiB buffer has been
rewritten (samples come from HBM).  Rounds are interleaved.  The derived figures come from the
launch times and the definition's counts: bytes = 4 * sum(len + out), fmas = K per output.

    python tools/resample_bench.py [--rounds 5] [--out FILE]

Prints one JSON line per rate pair (and writes them to --out).
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
import torch.nn.functional as F  # noqa: E402

from _bench import speech_like, timed_rounds  # noqa: E402

B, N_OUT = 16, 204544
PAIRS = [(48000, 22050), (44100, 22050)]


def conv_weight(bank, up, down, half):
    """[up, 1, 2 * half + down]: row r's taps start at column floor(r * down / up)."""
    K = 2 * half + 1
    w = torch.zeros(up, 1, 2 * half + down, dtype=bank.dtype, device=bank.device)
    for r in range(up):
        b = r * down // up
        w[r, 0, b:b + K] = bank[r, :K]
    return w


def torch_resample(x, w, up, down, half, n_out):
    periods = -(-n_out // up)
    need = (periods - 1) * down + w.shape[-1]
    xp = F.pad(x, (half, max(need - half - x.shape[1], 0)))
    y = F.conv1d(xp[:, None, :], w, stride=down)[:, :, :periods]       # [B, up, periods]
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :n_out]


def bench_pair(sr_in, sr_out, rounds, trash):
    import _resample_refs as R
    from tt2 import audio, ops
    dev = "cuda"
    rs = audio.Resampler(sr_in, sr_out)
    up, down, half = rs.up, rs.down, rs.half
    K = 2 * half + 1
    L = N_OUT * down // up
    assert rs.out_len(L) == N_OUT
    wav = speech_like(B, L).to(dev)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    y = torch.empty(B, N_OUT, device=dev)
    ol = torch.empty(B, dtype=torch.int32, device=dev)
    taps = rs.taps()
    w = conv_weight(taps, up, down, half)

    def resample():
        ops.resample(wav, y, taps, up, down, half, lens=lens, out_lens=ol)

    def resampler():
        rs(wav, lens)

    def torch_base():
        return torch_resample(wav, w, up, down, half, N_OUT)

    resample()
    base = torch_base()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = R.resample(wav[0].cpu().numpy(), L, taps.cpu().numpy(), up, down, half)
    numpy_s = time.perf_counter() - t0
    agree = {"torch_max_abs": float((base - y).abs().max()),
             "numpy_max_abs_utt0": float(np.abs(y[0].cpu().numpy().astype(np.float64) - ref).max()),
             "resampler_equal_bits": bool(torch.equal(rs(wav, lens)[0], y)),
             "peak": float(y.abs().max())}
    fns = {"resample": resample, "resampler": resampler, "torch": torch_base}
    res_us, evi_us = timed_rounds(fns, rounds, trash)
    best = {k: min(v) for k, v in res_us.items()}
    evi = {k: min(v) for k, v in evi_us.items()}
    nbytes = 4 * B * (L + N_OUT)
    fmas = B * N_OUT * K
    return {"pair": [sr_in, sr_out], "shape": dict(B=B, samples_in=L, samples_out=N_OUT, up=up, down=down, taps=K),
            "agree": agree, "rounds": rounds,
            "resident_us_best": {k: round(v, 2) for k, v in best.items()},
            "resident_us_median": {k: round(statistics.median(v), 2) for k, v in res_us.items()},
            "evicted_us_best": {k: round(v, 2) for k, v in evi.items()},
            "numpy_one_utterance_us": round(numpy_s * 1e6, 1),
            "derived": {"bytes": nbytes, "fmas": fmas,
                        "gb_per_s_resident": round(nbytes / (best["resample"] * 1e3), 1),
                        "gb_per_s_evicted": round(nbytes / (evi["resample"] * 1e3), 1),
                        "gfma_per_s_resident": round(fmas / (best["resample"] * 1e3), 1),
                        "speedup_vs_torch_resident": round(best["torch"] / best["resample"], 1),
                        "speedup_vs_torch_evicted": round(evi["torch"] / evi["resample"], 1)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    trash = torch.zeros(1 << 28, device="cuda")
    lines = []
    for sr_in, sr_out in PAIRS:
        lines.append(json.dumps(bench_pair(sr_in, sr_out, a.rounds, trash)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
