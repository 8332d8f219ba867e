"""Cost of MCD-DTW scoring on the GPU against what one had to do before (dev tool, GPU).

Shapes: B = 16 utterance pairs of 800 x 800 and 780 x 800 frames, 80-bin log-mels, 13 cepstral
coefficients (columns 1..13 of the 16-float cepstral rows).

* dtw:        the tt2_dtw launch alone, totals and lengths only;
* dtw_path:   the same with the path (move codes to the workspace, backtrack);
* dct:        the two DCT GEMMs (tt2.evaluate.mfcc of both sides);
* mcd_dtw:    the whole tt2.evaluate.mcd_dtw call (two GEMMs, tt2_dtw, the dB arithmetic), no path;
* torch_dp:   the baseline on the GPU: torch.cdist and a dynamic programme over the anti-diagonals,
              batched over the utterances (totals only; they are compared with tt2_dtw's first);
* numpy:      tests/_dtw_refs.py's anti-diagonal reference on ONE utterance, on the host.

Each GPU path is timed twice: "resident", ten back-to-back runs in a replayed hipGraph (inputs and
move codes stay in the caches), and "evicted", single runs between device events after a 1 GiB
buffer has been rewritten (inputs come from HBM).  Rounds are interleaved.  The per-tick and
per-backtrack-step figures are derived from the resident launch times and the kernel's schedule
(stages x ticks per stage; path cells), not from in-kernel counters.

    python tools/dtw_bench.py [--rounds 5]

Prints one JSON line per shape.
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

from _bench import timed_rounds, wall_us  # noqa: E402

B, NCOEF = 16, 13
CLOCK_GHZ = 2.4


def torch_dp(ch, cr):
    """Totals of the DTW of cepstral columns 1..13, batched, one step per anti-diagonal."""
    c = torch.cdist(ch[:, :, 1:NCOEF + 1], cr[:, :, 1:NCOEF + 1], compute_mode="donot_use_mm_for_euclid_dist")
    Bn, n, m = c.shape
    D = torch.full((Bn, n + 1, m + 1), float("inf"), device=c.device)
    D[:, 1, 1] = c[:, 0, 0]
    for d in range(1, n + m - 1):
        i = torch.arange(max(0, d - m + 1), min(n - 1, d) + 1, device=c.device)
        j = d - i
        best = torch.minimum(torch.minimum(D[:, i, j], D[:, i, j + 1]), D[:, i + 1, j])
        D[:, i + 1, j + 1] = c[:, i, j] + best
    return D[:, n, m]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from _dtw_refs import cost_ref, dtw_ref_fast
    from tt2 import evaluate, ops
    dev = "cuda"
    trash = torch.zeros(1 << 28, device=dev)
    for th, tr in ((800, 800), (780, 800)):
        torch.manual_seed(th)
        ref = torch.randn(B, tr, 80, device=dev) * 1.5 - 5.0
        # the decoded side: the reference resampled to th frames, plus noise
        idx = (torch.arange(th, device=dev).float() * (tr - 1) / max(th - 1, 1)).round().long()
        hyp = ref[:, idx] + 0.3 * torch.randn(B, th, 80, device=dev)
        ch, cr = evaluate.mfcc(hyp, NCOEF), evaluate.mfcc(ref, NCOEF)
        total = torch.empty(B, device=dev)
        length = torch.empty(B, dtype=torch.int32, device=dev)
        pa = torch.empty(B, th + tr - 1, dtype=torch.int32, device=dev)
        pb = torch.empty_like(pa)
        ws = ops.Workspace()
        cols = (1, NCOEF + 1)

        def dtw():
            ops.dtw(ch, cr, total, length, cols=cols)

        def dtw_path():
            ops.dtw(ch, cr, total, length, cols=cols, path_a=pa, path_b=pb, ws=ws)

        def dct():
            evaluate.mfcc(hyp, NCOEF), evaluate.mfcc(ref, NCOEF)

        def mcd():
            evaluate.mcd_dtw(hyp, None, ref, None, NCOEF)

        dtw_path()
        base = torch_dp(ch, cr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_total = dtw_ref_fast(cost_ref(ch[0].cpu().numpy(), cr[0].cpu().numpy(), 1, NCOEF + 1).astype(np.float64))[0]
        numpy_s = time.perf_counter() - t0
        agree = {"torch_dp_max_rel": float(((base - total).abs() / total).max()),
                 "numpy_rel_utt0": abs(float(total[0]) - n_total) / n_total,
                 "mean_path_cells": float(length.float().mean())}

        fns = {"dtw": dtw, "dtw_path": dtw_path, "dct": dct, "mcd_dtw": mcd}
        tdp = []
        res_us, evi_us = timed_rounds(fns, a.rounds, trash,
                                      each_round=lambda: tdp.append(wall_us(lambda: torch_dp(ch, cr))))
        best = {k: min(v) for k, v in res_us.items()}
        stages = (th + 31) // 32 + (tr + 63) // 64 - 1   # tb <= 1024: 32-row x 64-column tiles
        ticks = stages * (32 + 63)
        L = agree["mean_path_cells"]
        res = {"shape": dict(B=B, hyp=th, ref=tr, n_coef=NCOEF), "agree": agree, "rounds": a.rounds,
               "resident_us_best": {k: round(v, 2) for k, v in best.items()},
               "resident_us_median": {k: round(statistics.median(v), 2) for k, v in res_us.items()},
               "evicted_us_best": {k: round(min(v), 2) for k, v in evi_us.items()},
               "torch_dp_us_best": round(min(tdp), 1), "numpy_one_utterance_us": round(numpy_s * 1e6, 1),
               "derived": {"stages": stages, "ticks": ticks,
                           "cycles_per_tick_incl_costs": round(best["dtw"] * 1e3 * CLOCK_GHZ / ticks, 1),
                           "cycles_per_path_cell_moves_and_backtrack":
                               round((best["dtw_path"] - best["dtw"]) * 1e3 * CLOCK_GHZ / L, 1)},
               "speedup_vs_torch_dp": round(min(tdp) / best["dtw"], 1)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
