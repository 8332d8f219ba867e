"""Cost of the monotonic alignment search against the path it replaces (dev tool, GPU).

Shape: B=16, H=8, 800 frames x 128 phonemes, six layers, bf16, ragged lengths, best head per
utterance (align_bench.py's problem: queries peaked along the diagonal; layer 3 a little sharper
than the others, so every utterance's best head lies in one layer and the old path needs one
probability matrix).

* mono:        the tt2_align_monotonic launch alone (sel already on the device);
* mono_total:  tt2_attn_align (six layers) + tt2_align_durations + tt2_align_monotonic;
* argmax_total: the existing two-launch argmax path, beside them;
* old_total:   what one had to do before: tt2_attn_probs of the chosen layer (alignments()), the
               log of the chosen head's rows, and a torch dynamic programme on the GPU, batched
               over the utterances: 799 dependent rows forward, 799 dependent steps back.

The outputs are compared first (paths equal).  Each path is captured into a hipGraph and replayed;
rounds are interleaved.  The old path's graph holds one run (thousands of nodes), the others ten.

    python tools/mono_bench.py [--rounds 5]

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
SHARP = 3


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
    qs = []
    for l in range(L):
        q = torch.randn(B, TY, d, device=dev) * 0.5
        kk = mkv.view(B, TX, kvld)[:, :, 2 * d * l:2 * d * l + d].float()
        for b in range(B):
            n = torch.arange(TY, device=dev).clamp(max=int(qlen[b]) - 1)
            q[b] += (2.5 if l == SHARP else 2.0) * kk[b, (n * int(klen[b])) // int(qlen[b])]
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
    path = torch.empty(B, TY, device=dev, dtype=torch.int32)
    mdur = torch.empty(B, TX, device=dev, dtype=torch.int32)
    logp = torch.empty(B, device=dev)

    def argmax_total():
        ops.attn_align(qs, ks, lses, pmax, amax, d, kvld, B, H, TY, TX, key_len=klen, q_len=qlen, scale=0.125)
        ops.align_durations(pmax, amax, focus, sel, sel_focus, dur, L, B, H, TY, TX, key_len=klen, q_len=qlen)

    def mono():
        ops.align_monotonic(qs, ks, lses, path, mdur, logp, d, kvld, B, H, TY, TX, key_len=klen, q_len=qlen, sel=sel,
                            scale=0.125)

    def mono_total():
        argmax_total()
        mono()

    mono_total()
    torch.cuda.synchronize()
    assert (sel[:, 0] == SHARP).all(), sel[:, 0].tolist()

    probs = torch.empty(B, H, TY, TX, device=dev)
    bidx = torch.arange(B, device=dev)
    neg = torch.full((B, 1), float("-inf"), device=dev)
    te = torch.minimum(klen, qlen).long()
    ql = qlen.long()
    moves = torch.zeros(B, TY, TX, dtype=torch.bool, device=dev)
    opath = torch.empty(B, TY, dtype=torch.int64, device=dev)

    def old_total():
        ops.attn_probs(qs[SHARP], ks[SHARP], lses[SHARP], probs, d, kvld, B, H, TY, TX, key_len=klen, scale=0.125)
        lp = probs[bidx, sel[:, 1].long()].log()   # [B, TY, TX]; masked keys are -inf
        V = torch.cat([lp[:, 0, :1], neg.expand(B, TX - 1)], 1)
        for n in range(1, TY):
            prev = torch.cat([neg, V[:, :-1]], 1)
            moves[:, n] = prev > V
            V = torch.where((ql > n)[:, None], lp[:, n] + torch.maximum(V, prev), V)
        t = te - 1
        for n in range(TY - 1, -1, -1):
            act = ql > n
            opath[:, n] = torch.where(act, t, -1)
            t = t - (moves[:, n].gather(1, t[:, None])[:, 0] & act).long()

    old_total()
    torch.cuda.synchronize()
    agree = {"path_equal_share": (opath == path.long()).float().mean().item(),
             "durations_sum_ok": bool((mdur.sum(1) == qlen).all()),
             "min_duration": int(torch.stack([mdur[b, :int(klen[b])].min() for b in range(B)]).min()),
             "argmax_zero_durations": int(sum((dur[b, :int(klen[b])] == 0).sum() for b in range(B))),
             "logp_mean": logp.mean().item(), "focus_best_mean": sel_focus.mean().item()}

    graphs = {"mono": (graph_of(mono), 10), "mono_total": (graph_of(mono_total), 10),
              "argmax_total": (graph_of(argmax_total), 10), "old_total": (graph_of(old_total, n=1), 1)}
    us = {k: [] for k in graphs}
    for _ in range(a.rounds):   # interleaved: drift of the machine hits every path alike
        for k, (g, n) in graphs.items():
            us[k].append(time_graph(g, n=n, reps=5 if n > 1 else 2) * 1e6)
    res = {"shape": dict(B=B, H=H, Ty=TY, Tx=TX, layers=L, dtype="bf16"), "agree": agree,
           "us_best": {k: round(min(v), 2) for k, v in us.items()},
           "us_median": {k: round(statistics.median(v), 2) for k, v in us.items()}, "rounds": a.rounds,
           "speedup_best": round(min(us["old_total"]) / min(us["mono_total"]), 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
