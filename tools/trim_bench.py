"""Cost of silence trimming on the GPU against what one had to do before (dev tool, GPU).

Shape: B = 16 utterances of 204544 samples at 22.05 kHz (800 mel frames: the resampler benchmark's
output), 0.5 s of silence (low noise, 70 dB down) on each side of synthetic speech-like audio
(pitch_bench.py's), the defaults (top_db 60, frame 2048, hop 512, keep 0), n_out = n_in.

* trim:     the tt2_trim call alone (three launches) into preallocated buffers;
* trimmer:  the whole tt2.audio.SilenceTrimmer call (lengths to int32, three fresh tensors, the call);
* torch:    the baseline on the GPU with the same results: pad, unfold into frames, square and sum,
            amax, compare, argmax from both ends, gather (its start, lengths and samples are compared
            with tt2_trim's first);
* numpy:    tests/_trim_refs.py's float64 reference on ONE utterance, on the host.

Each GPU path is timed twice: "resident", ten back-to-back runs in a replayed hipGraph (the samples
stay in the caches), and "evicted", single runs between device events after a 1 GiB buffer has been
rewritten (samples come from HBM).  Rounds are interleaved.  The derived figures come from the call
times and the definition's counts: bytes = 4 * (sum(len) + B * n_out), each sample read once and each
output column written once.

    python tools/trim_bench.py [--rounds 5] [--out FILE]
    python tools/trim_bench.py --calls 200          # only tt2_trim calls, for a kernel trace

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
import torch.nn.functional as F  # noqa: E402

from _bench import HBM_GBPS, speech_like, timed_rounds  # noqa: E402

B, N, SR = 16, 204544, 22050


def padded_speech():
    """[B, N] f32: 0.5 s of noise 70 dB below the speech either side of it."""
    g = torch.Generator().manual_seed(1)
    pad = SR // 2
    wav = 1e-4 * torch.randn(B, N, generator=g)
    wav[:, pad:N - pad] = speech_like(B, N - 2 * pad)
    return wav


def torch_trim(x, lens, hop, r, keep, ratio):
    """(y, out_lens, start) by torch ops on the GPU; lens all equal to x.shape[1] here."""
    Bx, L = x.shape
    frame = 2 * r * hop
    Fn = 1 + L // hop
    xp = F.pad(x, (r * hop, r * hop + hop))
    e = xp.unfold(1, frame, hop)[:, :Fn].square().sum(-1)                 # [B, F]
    loud = e > ratio * e.amax(dim=1, keepdim=True)
    anyloud = loud.any(dim=1)
    f0 = loud.int().argmax(dim=1)
    f1 = Fn - 1 - loud.flip(1).int().argmax(dim=1)
    start = (f0 * hop - keep).clamp_min(0)
    end = torch.minimum(lens.long(), (f1 + 1) * hop + keep)
    start = torch.where(anyloud, start, torch.zeros_like(start))
    out = torch.where(anyloud, end - start, torch.zeros_like(start))
    col = torch.arange(L, device=x.device)[None, :]
    idx = (start[:, None] + col).clamp_max(L - 1)
    y = torch.where(col < out[:, None], x.gather(1, idx), torch.zeros((), device=x.device))
    return y, out.int(), start.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=0, help="only this many tt2_trim calls (for a kernel trace)")
    a = ap.parse_args()
    import _trim_refs as R
    from tt2 import audio, ops
    dev = "cuda"
    tr = audio.SilenceTrimmer()
    wav = padded_speech().to(dev)
    lens = torch.full((B,), N, dtype=torch.int32, device=dev)
    y = torch.empty(B, N, device=dev)
    ol = torch.empty(B, dtype=torch.int32, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    ws = ops.Workspace()

    def trim():
        ops.trim(wav, y, tr.hop, tr.r, tr.keep, tr.ratio, lens=lens, out_lens=ol, start=st, workspace=ws)

    def trimmer():
        tr(wav, lens)

    def torch_base():
        return torch_trim(wav, lens, tr.hop, tr.r, tr.keep, tr.ratio)

    if a.calls:
        for _ in range(a.calls):
            trim()
        torch.cuda.synchronize()
        return
    trim()
    ty, tol, tst = torch_base()
    torch.cuda.synchronize()
    x0 = wav[0].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.reference(x0[None, :], None, tr.hop, tr.r, tr.keep, np.float32(tr.ratio), N)
    numpy_s = time.perf_counter() - t0
    t = tr.trim(wav, lens)
    agree = {"torch_equal_bits": bool(torch.equal(ty, y) and torch.equal(tol, ol) and torch.equal(tst, st)),
             "numpy_equal_utt0": bool(int(ol[0]) == ref[1][0] and int(st[0]) == ref[2][0]
                                      and np.array_equal(y[0].cpu().numpy(), ref[0][0].astype(np.float32))),
             "trimmer_equal_bits": bool(torch.equal(t.audio, y) and torch.equal(t.lens, ol) and torch.equal(t.start, st)),
             "start": [int(st.min()), int(st.max())], "out_lens": [int(ol.min()), int(ol.max())]}
    fns = {"trim": trim, "trimmer": trimmer, "torch": torch_base}
    res_us, evi_us = timed_rounds(fns, a.rounds, torch.zeros(1 << 28, device=dev))
    best = {k: min(v) for k, v in res_us.items()}
    evi = {k: min(v) for k, v in evi_us.items()}
    nbytes = 4 * (int(lens.sum()) + B * N)
    floor_us = nbytes / (HBM_GBPS * 1e3)
    line = json.dumps({
        "shape": dict(B=B, samples=N, hop=tr.hop, frame=tr.frame, top_db=tr.top_db, keep=tr.keep, n_out=N),
        "agree": agree, "rounds": a.rounds,
        "resident_us_best": {k: round(v, 2) for k, v in best.items()},
        "resident_us_median": {k: round(statistics.median(v), 2) for k, v in res_us.items()},
        "evicted_us_best": {k: round(v, 2) for k, v in evi.items()},
        "numpy_one_utterance_us": round(numpy_s * 1e6, 1),
        "derived": {"bytes": nbytes, "hbm_floor_us": round(floor_us, 2),
                    "gb_per_s_resident": round(nbytes / (best["trim"] * 1e3), 1),
                    "gb_per_s_evicted": round(nbytes / (evi["trim"] * 1e3), 1),
                    "x_hbm_floor_resident": round(best["trim"] / floor_us, 1),
                    "x_hbm_floor_evicted": round(evi["trim"] / floor_us, 1),
                    "speedup_vs_torch_resident": round(best["torch"] / best["trim"], 1),
                    "speedup_vs_torch_evicted": round(evi["torch"] / evi["trim"], 1)}})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
