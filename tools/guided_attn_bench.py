"""Cost of the guided-attention loss (dev tool, GPU).

* the captured cfg2 training step (B=16, 128 phonemes / 800 frames, bf16, bench.py's model and
  optimizer setup) with guidance off and with it on at the defaults: two models of the same
  init, interleaved rounds of graph replays (ms per step, best and median of the rounds);
* the cross-attention forward and backward alone at tools/attn_bench.py's cross-attention shape
  (B=16, H=8, 800 queries x 128 keys), plain against guided with 2 and with 8 of 8 heads, and the
  loss reduction launch (six layers' rows), each as 10 launches replayed from a hipGraph.

    python tools/guided_attn_bench.py [--steps 20] [--rounds 5] [--kernels-only | --step-only]

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gemm_ab import graph_of, time_graph, ops  # noqa: E402

B, H, D, TX, TY = 16, 8, 64, 128, 800


def kernels():
    torch.manual_seed(0)
    d = H * D
    q = (torch.randn(B * TY, d, device="cuda") * 0.5).bfloat16()
    kv = (torch.randn(B * TX, 2 * d, device="cuda") * 0.5).bfloat16()
    k, v = kv, kv[:, d:]
    out = torch.empty(B * TY, d, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B * H, TY, device="cuda")
    rows = torch.zeros(B * H, TY, device="cuda")
    coef = torch.full((1,), 1e-6, device="cuda")
    klen = torch.full((B,), TX, dtype=torch.int32, device="cuda")
    qlen = torch.full((B,), TY, dtype=torch.int32, device="cuda")
    dout = (torch.randn(B * TY, d, device="cuda") * 0.1).bfloat16()
    dq = torch.empty(B * TY, d, device="cuda", dtype=torch.bfloat16)
    dkv = torch.empty(B * TX, 2 * d, device="cuda", dtype=torch.bfloat16)
    delta = torch.empty(B * H, TY, device="cuda")
    lds = (d, 2 * d, 2 * d, d, d, d, 2 * d, 2 * d)

    def us(fn):
        g = graph_of(fn)
        t = min(time_graph(g) for _ in range(3))
        del g
        return round(t * 1e6, 2)

    res = {"fwd_plain_us": us(lambda: ops.attn_fwd(q, k, v, out, lse, d, 2 * d, 2 * d, d, B, H, TY, TX, klen, False,
                                                   0.125)),
           "bwd_plain_us": us(lambda: ops.attn_bwd(q, k, v, out, dout, lse, delta, dq, dkv, dkv[:, d:], *lds, B, H, TY,
                                                   TX, klen, False, 0.125))}
    for gh in (2, 8):
        res[f"fwd_guided{gh}_us"] = us(lambda: ops.attn_fwd_guided(
            q, k, v, out, lse, rows, d, 2 * d, 2 * d, d, B, H, TY, TX, klen, q_len=qlen, guide_heads=gh))
        res[f"bwd_guided{gh}_us"] = us(lambda: ops.attn_bwd_guided(
            q, k, v, out, dout, lse, delta, dq, dkv, dkv[:, d:], rows, coef, *lds, B, H, TY, TX, klen, q_len=qlen,
            guide_heads=gh))
    six = [rows.clone() for _ in range(6)]
    term, loss = torch.zeros(1, device="cuda"), torch.zeros(4, device="cuda")
    res["loss_reduce_us"] = us(lambda: ops.guided_attn_loss(six, term, coef, B, H, TY, TX, key_len=klen, q_len=qlen,
                                                            loss_out=loss))
    return res


def captured_step(on: bool):
    """bench.py's model, optimizer setup and batch; three eager steps, then the captured step."""
    import bench
    from tt2.config import TTSConfig
    from tt2.model import TransformerTTS

    torch.manual_seed(0)
    m = TransformerTTS(TTSConfig(), dtype=torch.bfloat16)
    eng = m.engine
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(0)
        for name, (off, shape, n) in eng.lay.slots.items():
            if len(shape) >= 2:
                eng.P(name).copy_(torch.randn(shape, generator=g, device="cuda") / (n // shape[0]) ** 0.5)
            elif not (name.endswith(".g") or name.endswith("alpha")):
                eng.P(name).zero_()
        eng.sync_shadow()
    m.configure_optimizer(lr=1.0, warmup=4000.0, clip_norm=1.0)
    m.train()
    if on:
        m.guided_attention()
    batch = bench.synth_batch(0)
    for _ in range(3):
        m.train_step(*batch)
    run = m.capture_train_step(B, TX, TY)
    bufs = m.input_buffers(B, TX, TY)
    for dst, src in zip(bufs, batch):
        dst.copy_(src)
    return m, run, bufs


def time_steps(run, bufs, steps):
    run(*bufs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run(*bufs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    a = ap.parse_args()
    out = {}
    if not a.step_only:
        out["kernels"] = kernels()
    if not a.kernels_only:
        ms = {"off": [], "on": []}
        models = {"off": captured_step(False), "on": captured_step(True)}   # one model per setting, same init
        for _ in range(a.rounds):   # interleaved: drift of the box hits both alike
            for name, (m, run, bufs) in models.items():
                ms[name].append(time_steps(run, bufs, a.steps))
        out["step"] = {f"{k}_ms_best": round(min(v), 4) for k, v in ms.items()}
        out["step"].update({f"{k}_ms_median": round(statistics.median(v), 4) for k, v in ms.items()})
        out["step"]["delta_ms_median"] = round(statistics.median(ms["on"]) - statistics.median(ms["off"]), 4)
        out["step"]["guided_term"] = round(models["on"][0]._last["ga_term"].item(), 5)
        out["step"]["steps"], out["step"]["rounds"] = a.steps, a.rounds
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
