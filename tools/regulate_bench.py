"""Cost of the length regulator on the GPU against the two torch forms users write today (dev tool, GPU).

Shapes: B = 16, Tx = 128, n_out = 800 with D = 512 in bf16 (the hidden states), the same in f32, and
D = 1 in f32 (pitch / energy); random durations summing to 650 .. 800 frames per utterance.

Legs, each into preallocated tensors:
* plan:   tt2_regulate_plan (ends, index, frames, total);
* fwd:    tt2_regulate_fwd;
* bwd:    tt2_regulate_bwd;
* whole:  tt2.regulate.length_regulate (with max_frames) forward + autograd backward, fresh tensors.
Comparators on the GPU, checked to give the same values first:
* gather:  cumsum + searchsorted + gather + mask, and its autograd backward (a scatter-add with
           floating-point atomics: its bits vary run to run, which is measured too);
* repeat:  repeat_interleave per utterance + pad_sequence (a host synchronisation per utterance to
           learn the sizes; it cannot be captured into a graph), forward + backward.

Kernel legs are timed "resident" (ten back-to-back runs in a replayed hipGraph) and "evicted" (single
runs between device events after a 1 GiB buffer was rewritten); the whole-call legs eagerly (200
back-to-back calls between device events ending in a synchronise; host time included) and evicted.
Rounds are interleaved.  Bytes are the definition's: dtype * D * (rows read + rows written) plus
the int32 map.  The longest-phoneme experiment runs the backward on one utterance of 800 frames whose
128 durations are even (6 or 7 frames) against the same total with one phoneme of 400 frames.

    python tools/regulate_bench.py [--rounds 5] [--out FILE]
    python tools/regulate_bench.py --calls 200          # only the three kernels, for a kernel trace

Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from _bench import HBM_GBPS, timed_rounds  # noqa: E402

B, TX, N_OUT = 16, 128, 800
SHAPES = [("bf16_512", torch.bfloat16, 512), ("f32_512", torch.float32, 512), ("f32_1", torch.float32, 1)]


def random_durations(seed=0):
    """[B, TX] int32: every utterance sums to 650 .. 800 frames, some phonemes at 0."""
    g = torch.Generator().manual_seed(seed)
    d = torch.zeros(B, TX, dtype=torch.int64)
    for b in range(B):
        total = int(torch.randint(650, 801, (1,), generator=g))
        w = torch.rand(TX, generator=g) * (torch.rand(TX, generator=g) < 0.9)
        d[b] = torch.bincount(torch.multinomial(w, total, replacement=True, generator=g), minlength=TX)
    return d.to(torch.int32)


def torch_gather(h, d, n_out):
    """cumsum + searchsorted + gather + mask: no host synchronisation; autograd gives the backward."""
    ends = d.clamp(min=0).cumsum(1)
    n = torch.arange(n_out, device=h.device)[None, :].expand(h.shape[0], n_out).contiguous()
    idx = torch.searchsorted(ends, n, right=True)
    valid = n < ends[:, -1:]
    idx = idx.clamp(max=h.shape[1] - 1)
    y = torch.gather(h, 1, idx[:, :, None].expand(-1, -1, h.shape[2]))
    return y * valid[:, :, None].to(h.dtype)


def torch_repeat(h, d, n_out):
    """repeat_interleave per utterance + pad_sequence: the output size of every utterance is read on the host."""
    rows = [torch.repeat_interleave(h[b], d[b].clamp(min=0).long(), dim=0) for b in range(h.shape[0])]
    y = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True)
    return torch.nn.functional.pad(y, (0, 0, 0, n_out - y.shape[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=0, help="only this many calls of each kernel (for a kernel trace)")
    a = ap.parse_args()
    from tt2 import ops, regulate
    dev = "cuda"
    d = random_durations().to(dev)
    ends = torch.empty(B, TX, dtype=torch.int32, device=dev)
    index = torch.empty(B, N_OUT, dtype=torch.int32, device=dev)
    frames, total = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))

    def plan():
        ops.regulate_plan(d, N_OUT, ends=ends, index=index, frames=frames, total=total)

    plan()
    torch.cuda.synchronize()
    n_frames = int(frames.sum())
    bufs = {}
    for name, dtype, D in SHAPES:
        g = torch.Generator().manual_seed(D)
        bufs[name] = dict(h=torch.randn(B, TX, D, generator=g).to(dev, dtype), dy=torch.randn(B, N_OUT, D, generator=g).to(dev, dtype),
                          y=torch.empty(B, N_OUT, D, dtype=dtype, device=dev), dh=torch.empty(B, TX, D, dtype=dtype, device=dev))
    fns = {"plan": plan}
    nbytes = {"plan": 4 * (B * TX * 2 + B * N_OUT + 2 * B)}
    agree = {}
    for name, dtype, D in SHAPES:
        t = bufs[name]
        es = t["h"].element_size()
        fns[f"fwd_{name}"] = lambda t=t: ops.regulate_fwd(t["h"], index, t["y"])
        fns[f"bwd_{name}"] = lambda t=t: ops.regulate_bwd(t["dy"], ends, t["dh"])
        # rows read + rows written, and the map
        nbytes[f"fwd_{name}"] = es * D * (n_frames + B * N_OUT) + 4 * B * N_OUT
        nbytes[f"bwd_{name}"] = es * D * (n_frames + B * TX) + 4 * B * TX

        def whole(t=t):
            h = t["h"].detach().requires_grad_()
            regulate.length_regulate(h, d, max_frames=N_OUT).out.backward(t["dy"])
            return h.grad

        def gather(t=t):
            h = t["h"].detach().requires_grad_()
            torch_gather(h, d, N_OUT).backward(t["dy"])
            return h.grad

        def repeat(t=t):
            h = t["h"].detach().requires_grad_()
            torch_repeat(h, d, N_OUT).backward(t["dy"])
            return h.grad

        fns[f"whole_{name}"], fns[f"gather_{name}"], fns[f"repeat_{name}"] = whole, gather, repeat
        fns[f"gather_fwd_{name}"] = lambda t=t: torch_gather(t["h"], d, N_OUT)
        if a.calls:
            continue
        # the same values first: forward bit for bit, backward to the rounding of a different order
        fns[f"fwd_{name}"]()
        y_g, y_r = torch_gather(t["h"], d, N_OUT), torch_repeat(t["h"], d, N_OUT)
        g_ours, g_g, g_r = whole().float(), gather().float(), repeat().float()
        grads_g = torch.stack([gather().float() for _ in range(4)])
        scale = g_ours.abs().max().item()
        agree[name] = {"fwd_equal_bits": bool(torch.equal(t["y"], y_g) and torch.equal(t["y"], y_r)),
                       "bwd_max_diff_over_max": [round((g_ours - x).abs().max().item() / scale, 6) for x in (g_g, g_r)],
                       "ours_equal_bits_4_runs": all(bool(torch.equal(whole().float(), g_ours)) for _ in range(4)),
                       "gather_bwd_elements_varying_4_runs": int((grads_g != grads_g[0]).any(0).sum())}
    if a.calls:
        for _ in range(a.calls):
            for k in ("plan", "fwd_bf16_512", "bwd_bf16_512", "fwd_f32_512", "bwd_f32_512", "fwd_f32_1", "bwd_f32_1"):
                fns[k]()
        torch.cuda.synchronize()
        return
    # the longest phoneme: one utterance of 800 frames, even durations against one phoneme of 400
    even = torch.full((1, TX), 6, dtype=torch.int32)
    even[0, :800 - 6 * TX] += 1
    skew = torch.full((1, TX), 3, dtype=torch.int32)
    skew[0, :400 - 3 * (TX - 1)] += 1
    skew[0, TX // 2] = 400
    skew[0, TX - 1] -= int(skew.sum()) - 800
    tails = {}
    for nm, dd in (("even", even), ("skew", skew)):
        assert int(dd.sum()) == 800 and int(dd.min()) >= 0
        e1 = torch.empty(1, TX, dtype=torch.int32, device=dev)
        ops.regulate_plan(dd.to(dev), N_OUT, ends=e1)
        dy1, dh1 = bufs["bf16_512"]["dy"][:1], torch.empty(1, TX, 512, dtype=torch.bfloat16, device=dev)
        tails[nm] = (lambda e1=e1, dy1=dy1, dh1=dh1: ops.regulate_bwd(dy1, e1, dh1))
        fns[f"bwd_one_utt_{nm}"] = tails[nm]
    kernel_legs = [k for k in fns if k.startswith(("plan", "fwd_", "bwd_", "gather_fwd_"))]
    eager_legs = [k for k in fns if k.startswith(("whole_", "gather_", "repeat_")) and not k.startswith("gather_fwd_")]
    assert set(kernel_legs) | set(eager_legs) == set(fns)
    all_us, evi_us = timed_rounds(fns, a.rounds, torch.zeros(1 << 28, device=dev), eager=eager_legs, eager_runs=200)
    res_us = {k: all_us[k] for k in kernel_legs}
    eag_us = {k: all_us[k] for k in eager_legs}
    best = {k: min(v) for k, v in res_us.items()}
    eag = {k: min(v) for k, v in eag_us.items()}
    evi = {k: min(v) for k, v in evi_us.items()}
    derived = {}
    for name, _, _ in SHAPES:
        derived[name] = {
            "fwd_gb_per_s_resident": round(nbytes[f"fwd_{name}"] / (best[f"fwd_{name}"] * 1e3), 1),
            "bwd_gb_per_s_resident": round(nbytes[f"bwd_{name}"] / (best[f"bwd_{name}"] * 1e3), 1),
            "fwd_gb_per_s_evicted": round(nbytes[f"fwd_{name}"] / (evi[f"fwd_{name}"] * 1e3), 1),
            "bwd_gb_per_s_evicted": round(nbytes[f"bwd_{name}"] / (evi[f"bwd_{name}"] * 1e3), 1),
            "fwd_x_hbm_floor_resident": round(best[f"fwd_{name}"] / (nbytes[f"fwd_{name}"] / (HBM_GBPS * 1e3)), 1),
            "gather_fwd_over_fwd_resident": round(best[f"gather_fwd_{name}"] / best[f"fwd_{name}"], 1),
            "gather_over_whole_eager": round(eag[f"gather_{name}"] / eag[f"whole_{name}"], 2),
            "repeat_over_whole_eager": round(eag[f"repeat_{name}"] / eag[f"whole_{name}"], 2)}
    derived["bwd_one_utt_skew_over_even_resident"] = round(best["bwd_one_utt_skew"] / best["bwd_one_utt_even"], 2)
    line = json.dumps({
        "shape": dict(B=B, Tx=TX, n_out=N_OUT, frames=n_frames, frames_min=int(frames.min()), frames_max=int(frames.max()),
                      longest_phoneme=int(d.max())),
        "agree": agree, "rounds": a.rounds, "bytes": nbytes,
        "resident_us_best": {k: round(v, 2) for k, v in best.items()},
        "resident_us_median": {k: round(statistics.median(v), 2) for k, v in res_us.items()},
        "eager_us_best": {k: round(v, 2) for k, v in eag.items()},
        "evicted_us_best": {k: round(v, 2) for k, v in evi.items()},
        "derived": derived})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
