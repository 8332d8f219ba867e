"""Cost of the forward-sum alignment loss on the GPU against the torch stand-ins (dev tool, GPU).

Shape: B = 16, Ty = 800 frames, Tx = 128 phonemes, every utterance full length; near-diagonal random
scores (tests/_fsum_refs.py's "random" problem, tiled).

Legs, each into preallocated tensors:
* fwd:        tt2_forward_sum_fwd (loss, lse, alpha);   fwd_loss_only: the same with alpha NULL;
* bwd:        tt2_forward_sum_bwd (the beta walk and the element-parallel launch; dscores);
* path:       tt2_forward_sum_path;
* (tt2_align_monotonic is not run here: DESIGN.md 5.5 has its 109 us at this shape;)
* whole:      tt2.forward_sum.forward_sum_loss forward + autograd backward, fresh tensors.
Comparators on the GPU, checked to give the same loss and gradient first:
* ctc_batched:  F.ctc_loss on cat(blank column at -1e4, log_softmax(scores)), one call for the batch,
                forward + backward;
* ctc_loop:     the per-utterance loop of the published recipes (one F.ctc_loss call per utterance),
                forward + backward.

Kernel legs are timed "resident" (ten back-to-back runs in a replayed hipGraph) and "evicted" (single
runs between device events after a 1 GiB buffer was rewritten); the whole-call legs eagerly (back-to-
back calls between device events ending in a synchronise; host time included) and evicted.  Rounds
are interleaved.

    python tools/forward_sum_bench.py [--rounds 5] [--out FILE]

Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from _bench import timed_rounds  # noqa: E402

B, TY, TX = 16, 800, 128
BLANK = -1e4


def ctc_batched(s):
    """-ln Z per utterance through F.ctc_loss with a blank nobody can afford (full lengths)."""
    lp = torch.cat((s.new_full((B, TY, 1), BLANK), torch.log_softmax(s, 2)), 2).transpose(0, 1)
    tgt = torch.arange(1, TX + 1, device=s.device)[None].expand(B, TX)
    lens = (torch.full((B,), TY, dtype=torch.long), torch.full((B,), TX, dtype=torch.long))
    return Fn.ctc_loss(lp, tgt, lens[0], lens[1], blank=0, reduction="none", zero_infinity=True)


def ctc_loop(s):
    out = []
    tgt = torch.arange(1, TX + 1, device=s.device)[None]
    for b in range(B):
        lp = torch.cat((s.new_full((TY, 1), BLANK), torch.log_softmax(s[b], 1)), 1)[:, None]
        out.append(Fn.ctc_loss(lp, tgt, torch.tensor([TY]), torch.tensor([TX]), blank=0, reduction="sum", zero_infinity=True))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _fsum_refs as R
    from tt2 import forward_sum as FS, ops
    dev = "cuda"
    rng = R.np.random.default_rng(0)
    n, t = R.np.arange(TY)[:, None], R.np.arange(TX)[None, :]
    s = torch.from_numpy((rng.standard_normal((B, TY, TX)) - 8.0 * (t / TX - n / TY) ** 2).astype("float32")).to(dev)
    loss, logp = (torch.empty(B, device=dev) for _ in range(2))
    lse = torch.empty(B, TY, device=dev)
    alpha, ds = (torch.empty(B, TY, TX, device=dev) for _ in range(2))
    path = torch.empty(B, TY, dtype=torch.int32, device=dev)
    dur = torch.empty(B, TX, dtype=torch.int32, device=dev)
    up = torch.linspace(0.5, 1.5, B, device=dev)

    def whole():
        x = s.detach().requires_grad_()
        (FS.forward_sum_loss(x, reduction="none") * up).sum().backward()
        return x.grad

    def with_grad(f):
        def run():
            x = s.detach().requires_grad_()
            (f(x) * up).sum().backward()
            return x.grad
        return run

    fns = {"fwd": lambda: ops.forward_sum_fwd(s, loss, lse, alpha),
           "fwd_loss_only": lambda: ops.forward_sum_fwd(s, loss, lse),
           "bwd": lambda: ops.forward_sum_bwd(s, lse, alpha, dscores=ds, grad_loss=up),
           "path": lambda: ops.forward_sum_path(s, path, dur, logp),
           "whole": whole, "ctc_batched": with_grad(ctc_batched), "ctc_loop": with_grad(ctc_loop)}
    # the same values first
    fns["fwd"]()
    ours, g_ours = loss.clone(), whole()
    l_b, l_l = ctc_batched(s), ctc_loop(s)
    g_b, g_l = fns["ctc_batched"](), fns["ctc_loop"]()
    r64 = R.forward_sum(s[0].cpu().numpy(), TY, TX)
    scale = g_ours.abs().max().item()
    agree = {"loss_rel_diff_ctc_batched": float(((ours - l_b).abs() / ours.abs()).max()),
             "loss_rel_diff_ctc_loop": float(((ours - l_l).abs() / ours.abs()).max()),
             "grad_max_diff_over_max": [round((g_ours - x).abs().max().item() / scale, 8) for x in (g_b, g_l)],
             "loss_rel_err_float64_utt0": {"ours": abs(ours[0].item() - r64["loss"]) / r64["loss"],
                                           "ctc_batched": abs(l_b[0].item() - r64["loss"]) / r64["loss"]},
             "grad_max_err_float64_utt0": {
                 "ours": float(R.np.abs(g_ours[0].cpu().numpy() / up[0].item() - r64["grad"]).max()),
                 "ctc_batched": float(R.np.abs(g_b[0].cpu().numpy() / up[0].item() - r64["grad"]).max())},
             "ours_equal_bits_4_runs": all(bool(torch.equal(whole(), g_ours)) for _ in range(4)),
             "ctc_batched_grad_equal_bits_4_runs": all(bool(torch.equal(fns["ctc_batched"](), g_b)) for _ in range(4))}
    eager_legs = ["whole", "ctc_batched", "ctc_loop"]
    all_us, evi_us = timed_rounds(fns, a.rounds, torch.zeros(1 << 28, device=dev), eager=eager_legs, eager_runs=20)
    best = {k: min(v) for k, v in all_us.items()}
    evi = {k: min(v) for k, v in evi_us.items()}
    line = json.dumps({
        "shape": dict(B=B, Ty=TY, Tx=TX), "agree": agree, "rounds": a.rounds,
        "us_best": {k: round(v, 2) for k, v in best.items()},
        "us_median": {k: round(statistics.median(v), 2) for k, v in all_us.items()},
        "evicted_us_best": {k: round(v, 2) for k, v in evi.items()},
        "derived": {"fwd_ns_per_row": round(best["fwd"] * 1e3 / TY, 1), "path_ns_per_row": round(best["path"] * 1e3 / TY, 1),
                    "fwd_plus_bwd_us": round(best["fwd"] + best["bwd"], 2),
                    "ctc_batched_over_whole": round(best["ctc_batched"] / best["whole"], 2),
                    "ctc_loop_over_whole": round(best["ctc_loop"] / best["whole"], 2)},
        "legs": {"resident_graph": ["fwd", "fwd_loss_only", "bwd", "path"], "eager": eager_legs}})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
