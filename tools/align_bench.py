"""Cost of the fused alignment statistics against the path they replace (dev tool, GPU).

Shape: B=16, H=8, 800 frames x 128 phonemes, six layers, bf16 (the benchmark workload's
encoder-decoder attention; K of layer l is a column slice of one wide buffer, as mkv is).

* new: one tt2_attn_align launch for the six layers + one tt2_align_durations launch;
* old: six tt2_attn_probs launches (the [B, H, Ty, Tx] f32 matrix of each layer), then torch
  amax / argmax over the keys, the masked mean over the frames, the best head per utterance
  and a scatter_add of the chosen head's argmax into durations;
* for scale: the cross-attention forward of one layer at the same shape.

Outputs are compared first (argmax, best head and durations equal, pmax / focus close).  Each
path is captured into a hipGraph and replayed; rounds are interleaved.  The replays run over the
same buffers, which stay in the last-level cache; "us_cold_median" repeats the new path and the
forward with a 1 GiB fill in front of every launch (the fill's own time subtracted), which is
what a call right after a training step sees.

    python tools/align_bench.py [--rounds 5]

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gemm_ab import graph_of, time_graph, ops  # noqa: E402

B, H, D, TX, TY, L = 16, 8, 64, 128, 800, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    torch.manual_seed(0)
    d = H * D
    dev = "cuda"
    kvld = L * 2 * d
    klen = torch.randint(TX // 2, TX + 1, (B,), dtype=torch.int32, device=dev)
    qlen = torch.randint(TY // 2, TY + 1, (B,), dtype=torch.int32, device=dev)
    klen[0], qlen[0] = TX, TY
    mkv = (torch.randn(B * TX, kvld, device=dev) * 0.5).bfloat16()
    # queries that look along the diagonal, as a trained head does
    qs = []
    n = torch.arange(TY, device=dev)
    for l in range(L):
        q = torch.randn(B, TY, d, device=dev) * 0.5
        kk = mkv.view(B, TX, kvld)[:, :, 2 * d * l:2 * d * l + d].float()
        for b in range(B):
            q[b] += 2.0 * kk[b, (n * int(klen[b])) // TY]
        qs.append(q.view(B * TY, d).bfloat16())
    ks = [mkv[:, 2 * d * l:] for l in range(L)]
    vs = [mkv[:, 2 * d * l + d:] for l in range(L)]
    out = torch.empty(B * TY, d, device=dev, dtype=torch.bfloat16)
    lses = [torch.empty(B * H, TY, device=dev) for _ in range(L)]
    for l in range(L):
        ops.attn_fwd(qs[l], ks[l], vs[l], out, lses[l], d, kvld, kvld, d, B, H, TY, TX, klen, False, 0.125)

    pmax = torch.empty(L, B, H, TY, device=dev)
    amax = torch.empty(L, B, H, TY, device=dev, dtype=torch.int32)
    focus = torch.empty(L, B, H, device=dev)
    sel = torch.empty(B, 2, device=dev, dtype=torch.int32)
    sel_focus = torch.empty(B, device=dev)
    dur = torch.empty(B, TX, device=dev, dtype=torch.int32)

    def new_align():
        ops.attn_align(qs, ks, lses, pmax, amax, d, kvld, B, H, TY, TX, key_len=klen, q_len=qlen, scale=0.125)

    def new_dur():
        ops.align_durations(pmax, amax, focus, sel, sel_focus, dur, L, B, H, TY, TX, key_len=klen, q_len=qlen)

    def new():
        new_align()
        new_dur()

    probs = torch.empty(L, B, H, TY, TX, device=dev)
    valid = (torch.arange(TY, device=dev)[None, :] < qlen[:, None])
    o = {}
    bidx = torch.arange(B, device=dev)

    def old_probs():
        for l in range(L):
            ops.attn_probs(qs[l], ks[l], lses[l], probs[l], d, kvld, B, H, TY, TX, key_len=klen, scale=0.125)

    def old_torch():
        pm = probs.amax(-1) * valid[None, :, None, :]
        am = probs.argmax(-1)
        fc = pm.sum(-1) / qlen[None, :, None].clamp(min=1)
        flat = fc.permute(1, 0, 2).reshape(B, L * H).argmax(-1)
        rows = am.permute(1, 0, 2, 3).reshape(B, L * H, TY)[bidx, flat]
        o["dur"] = torch.zeros(B, TX, device=dev, dtype=torch.int64).scatter_add_(1, rows, valid.long())
        o["pm"], o["am"], o["fc"], o["flat"] = pm, am, fc, flat

    def old():
        old_probs()
        old_torch()

    # ---- the two paths agree
    new()
    old()
    torch.cuda.synchronize()
    vm = valid[None, :, None, :].expand(L, B, H, TY)
    am_eq = (amax.long() == o["am"])[vm].float().mean().item()
    agree = {
        "argmax_equal_share": am_eq,
        "pmax_rel": ((pmax - o["pm"]).norm() / o["pm"].norm()).item(),
        "focus_max_abs": (focus - o["fc"]).abs().max().item(),
        "best_head_equal": bool((sel[:, 0].long() * H + sel[:, 1].long() == o["flat"]).all()),
        "durations_l1": int((dur.long() - o["dur"]).abs().sum()),
        "focus_mean": focus.mean().item(), "focus_best_mean": sel_focus.mean().item(),
    }

    def fwd1():
        ops.attn_fwd(qs[0], ks[0], vs[0], out, lses[0], d, kvld, kvld, d, B, H, TY, TX, klen, False, 0.125)

    graphs = {"new_total": graph_of(new), "new_align": graph_of(new_align), "new_durations": graph_of(new_dur),
              "old_total": graph_of(old), "old_probs6": graph_of(old_probs), "old_torch": graph_of(old_torch),
              "fwd_one_layer": graph_of(fwd1)}
    # cold: a 1 GiB fill in front of every launch pushes the inputs out of the last-level cache (the
    # warm graphs above replay over the same 99 MB, which stays resident); the fill's own time
    # is measured alone and subtracted
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)

    def cold(fn):
        def run():
            flush.zero_()
            fn()
        return run

    graphs.update({"flush": graph_of(flush.zero_), "cold_new_align+flush": graph_of(cold(new_align)),
                   "cold_new_total+flush": graph_of(cold(new)), "cold_fwd_one_layer+flush": graph_of(cold(fwd1))})
    us = {k: [] for k in graphs}
    for _ in range(a.rounds):   # interleaved: drift of the machine hits every path alike
        for k, g in graphs.items():
            us[k].append(time_graph(g) * 1e6)
    res = {"shape": dict(B=B, H=H, Ty=TY, Tx=TX, layers=L, dtype="bf16"), "agree": agree,
           "us_best": {k: round(min(v), 2) for k, v in us.items()},
           "us_median": {k: round(statistics.median(v), 2) for k, v in us.items()},
           "us_cold_median": {k[5:-6]: round(statistics.median(us[k]) - statistics.median(us["flush"]), 2)
                              for k in us if k.startswith("cold_")},
           "align_per_layer_us": round(min(us["new_align"]) / L, 2), "rounds": a.rounds,
           "speedup_best": round(min(us["old_total"]) / min(us["new_total"]), 2)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
