"""Cost of Viterbi pitch tracking on the GPU against what one had to do before (dev tool, GPU).

Shape: B = 16 and B = 64 utterances of 800 frames (204544 samples each at hop 256), lags 37..339
(303 lag states and the unvoiced one), jump 1, switch 0.1, unvoiced 0.2, pos = log2: per frame
303 x 303 (from, to) pairs of one subtract, one fma and one min each.

* track:      the tt2_pitch_track launch alone on a d' tensor that tt2_yin wrote;
* tracker:    the whole tt2.audio.PitchTracker call (tt2_reflect_pad, the frame counts, the result
              tensors and the d' tensor, tt2_yin writing d', tt2_pitch_track);
* extractor:  the whole tt2.audio.PitchExtractor call, for what tracking adds;
* torch:      the same recurrence with torch ops on the GPU at B = 16: a frame loop over a
              [B, S, S] broadcast min with the predecessors recorded, then a frame loop back (its
              lags are compared with tt2_pitch_track's first, and must be the same);
* numpy:      tests/_pitch_track_refs.py's float64 reference on ONE utterance, on the host.

Each GPU path is timed twice: "resident", ten back-to-back runs in a replayed hipGraph, and
"evicted", single runs between device events after a 1 GiB buffer has been rewritten (d' comes
from HBM).  Rounds are interleaved.  The derived figures (share of the VALU issue rate of the CUs
in use) come from the resident launch time and the operation count of the definition, not from
in-kernel counters: one work group per utterance, so B of the 256 CUs work.

    python tools/pitch_track_bench.py [--rounds 5] [--out FILE]

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

T = 800
CLOCK_GHZ = 2.4


def torch_track(cm, lo, hi, pos, J, W, C):
    """The recurrence of tt2_pitch_track with torch ops, every utterance with all T frames ->
    lag [B, T] int64 (0 unvoiced).  X = V + J |dp| is two rounded operations where the kernel has
    one fma."""
    c = cm[:, :, lo:hi + 1]
    B, T_, S = c.shape
    p = pos[lo:hi + 1]
    JD = (J * (p[:, None] - p[None, :]).abs())[None]          # [1, to, from]
    V = c[:, 0]
    U = torch.full((B,), C, device=cm.device)
    from_v = torch.empty(B, T_, S, dtype=torch.int64, device=cm.device)
    from_u = torch.empty(B, T_, dtype=torch.int64, device=cm.device)
    for f in range(1, T_):
        A, arg = (V[:, None, :] + JD).min(dim=2)
        uw = (U + W)[:, None]
        take_u = uw < A
        m, m_arg = V.min(dim=1)
        mw = m + W
        take_v = mw < U
        from_v[:, f] = torch.where(take_u, -1, arg)
        from_u[:, f] = torch.where(take_v, m_arg, -1)
        V = c[:, f] + torch.where(take_u, uw, A)
        U = C + torch.where(take_v, mw, U)
    m, st = V.min(dim=1)
    st = torch.where(U < m, -1, st)
    states = torch.empty(B, T_, dtype=torch.int64, device=cm.device)
    for f in range(T_ - 1, -1, -1):
        states[:, f] = st
        if f:
            st = torch.where(st < 0, from_u[:, f], from_v[:, f].gather(1, st.clamp_min(0)[:, None])[:, 0])
    return torch.where(states < 0, 0, states + lo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _pitch_track_refs as R
    from tt2 import audio, ops
    dev = "cuda"
    L = (T - 1) * 256
    mx = audio.MelExtractor()
    px = audio.PitchExtractor(mx)
    tr = audio.PitchTracker(px)
    lo, hi, S = tr.tau_min, tr.tau_max, tr.tau_max - tr.tau_min + 1
    J, W, C = tr.jump, tr.switch, tr.unvoiced
    fns, keep, agree = {}, [], {}
    for B in (16, 64):
        wav = speech_like(B, L).to(dev)
        whole = tr.track(wav)
        plain = px(wav)
        _, _, _, _, frames, cm = px._yin(wav, None, True)
        f0 = torch.empty(B, T, device=dev)
        lag = torch.empty(B, T, dtype=torch.int32, device=dev)
        cost = torch.empty(B, device=dev)
        keep.append((wav, cm, f0, lag, cost, frames))

        def track(cm=cm, frames=frames, f0=f0, lag=lag, cost=cost):
            ops.pitch_track(cm, frames, f0, lag, cost, lo, hi, 22050.0, tr.pos(), J, W, C)

        def tracker(wav=wav):
            tr.track(wav)

        track()
        torch.cuda.synchronize()
        assert torch.equal(lag, whole.lag) and torch.equal(f0.view(torch.int32), whole.pitch.f0.view(torch.int32))
        fns[f"track_b{B}"], fns[f"tracker_b{B}"] = track, tracker
        if B == 16:
            fns["extractor_b16"] = lambda wav=wav: px(wav)
            base = torch_track(cm, lo, hi, tr.pos(), J, W, C)
            torch.cuda.synchronize()
            assert torch.equal(base, lag.long()), "the torch recurrence and tt2_pitch_track disagree on a lag"
            cm0 = cm[0].cpu().numpy()
            t0 = time.perf_counter()
            ref = R.track(cm0, lo, hi, R.log2_pos(), J, W, C, dtype=np.float64)
            numpy_s = time.perf_counter() - t0
            k_lag = lag[0].cpu().numpy()
            agree = {"torch_lags_equal": True, "numpy_lag_equal_utt0": float((ref["lag"] == k_lag).mean()),
                     "numpy_cost_rel_utt0": abs(float(cost[0]) - float(ref["cost"])) / float(ref["cost"]),
                     "voiced_share_tracker": float((lag > 0).float().mean()),
                     "voiced_share_extractor": float(plain.voiced.float().mean()),
                     "frames_where_voicing_differs": float(((lag > 0) != plain.voiced).float().mean())}
            torch_args = (cm, lo, hi, tr.pos(), J, W, C)

    tdp = []
    res_us, evi_us = timed_rounds(fns, a.rounds, torch.zeros(1 << 28, device=dev),
                                  each_round=lambda: tdp.append(wall_us(lambda: torch_track(*torch_args))))
    best = {k: min(v) for k, v in res_us.items()}
    pairs = (T - 1) * S * S                          # per utterance: one subtract, one fma, one min each
    floor = 3 * pairs / (4 * 32 * CLOCK_GHZ * 1e3)   # us: one CU per utterance, 4 SIMDs of 32 lanes per clock
    res = {"shape": dict(frames=T, samples=L, tau_min=lo, tau_max=hi, states=S + 1, jump=J, switch=W, unvoiced=C),
           "agree": agree, "rounds": a.rounds,
           "resident_us_best": {k: round(v, 1) for k, v in best.items()},
           "resident_us_median": {k: round(statistics.median(v), 1) for k, v in res_us.items()},
           "evicted_us_best": {k: round(min(v), 1) for k, v in evi_us.items()},
           "torch_b16_us_best": round(min(tdp), 1), "numpy_one_utterance_us": round(numpy_s * 1e6, 1),
           "derived": {"pairs_per_utterance": pairs, "valu_floor_us_one_cu_per_utterance": round(floor, 1),
                       "share_of_valu_issue_b16": round(floor / best["track_b16"], 3),
                       "us_per_frame_b16": round(best["track_b16"] / T, 3),
                       "workspace_mb": {f"b{B}": round(B * T * (S + 1) * 4 / 1e6, 1) for B in (16, 64)}},
           "speedup_vs_torch_b16": round(min(tdp) / best["track_b16"], 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
