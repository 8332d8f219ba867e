"""Cost of Gaussian upsampling on the GPU against the composed torch form (dev tool, GPU).

Shapes: B = 16, Tx = 128, n_out = 800, D = 512 in bf16 and in f32; random durations summing to
650 .. 800 frames per utterance (regulate_bench's), delta = 0.1, offset 0 (ESPnet's convention).

Legs, the kernel ones into preallocated tensors:
* fwd:     tt2_gauss_upsample_fwd (y, lse);
* bwd:     tt2_gauss_upsample_bwd asked for dh, dcenter and dprec (three launches: delta, the pass, the
           reduction of the 7 partials per phoneme tile);
* bwd_dh:  the same asked for dh alone (two launches: the pass and the reduction);
* whole:   tt2.upsample.gaussian_upsample (with max_frames) forward + autograd backward into h, the
           float durations and a delta tensor, fresh tensors;
* torch:   ESPnet's GaussianUpsampling as composed torch (arange, cumsum, a broadcast square,
           masked_fill, softmax, matmul) with its autograd backward into the same three, on the same
           GPU in the same process, checked against the fused form first; its frames past mel_len
           are multiplied by 0 (one more [B, n_out, D] pass each way than ESPnet's own form, which
           leaves the row of phoneme 0 there), so that the two compute the same values;
* espnet:  ESPnet's own form, without that mask (text_len is full here, so its masked_fill over the
           phonemes is left out as well): the cheapest torch form, the one the ratios are taken against.

Kernel legs are timed "resident" (ten back-to-back runs in a replayed hipGraph) and "evicted" (single
runs between device events after a 1 GiB buffer was rewritten); the whole-call legs eagerly (back-to-back
calls between device events ending in a synchronise; host time included) and evicted.  Rounds are
interleaved.  Bytes are the definition's: every row of h, dy and y read once, every row of y / dh
written once.  FLOP are the two (forward) or four (backward) matrix products' only.  Peak memory is
torch's max_memory_allocated over one forward + backward above what the inputs hold, plus, for the
fused form, the backward's workspace (tt2_gauss_upsample_bwd_workspace_size: delta and the f32
partials of the frame split), which lives in the module's persistent scratch buffer.  The tile figure
is the share of the forward's 64-frame x 32-phoneme tiles (inside the utterances) in which no weight
exceeds 2^-24: what a later band-skipping kernel could leave out.

    python tools/upsample_bench.py [--rounds 5] [--out FILE]

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
from regulate_bench import random_durations  # noqa: E402

B, TX, N_OUT, D = 16, 128, 800, 512
SHAPES = [("bf16", torch.bfloat16), ("f32", torch.float32)]
BF16_MFMA_TFLOPS = 2500.0      # dense peak of one MI355X; f32-input MFMA and the f32 vector ALU: 157.3
F32_TFLOPS = 157.3


def composed(h, d, mel_len, n_out, delta):
    """ESPnet's GaussianUpsampling; mel_len given: frames at and past it masked to 0 as the fused form
    leaves them."""
    c = torch.cumsum(d, 1) - d / 2
    t = torch.arange(n_out, device=h.device, dtype=d.dtype)
    e = -delta[:, None, :] * (t[None, :, None] - c[:, None, :]) ** 2
    w = torch.softmax(e, dim=2)
    y = torch.matmul(w.to(h.dtype), h)
    if mel_len is None:
        return y
    return y * (torch.arange(n_out, device=h.device)[None] < mel_len[:, None])[:, :, None].to(h.dtype)


def empty_tile_share(d, mel_len, delta=0.1):
    """Share of 64 x 32 (frame, phoneme) tiles inside the utterances whose largest weight is <= 2^-24."""
    d = d.double()
    c = torch.cumsum(d, 1) - d / 2
    t = torch.arange(N_OUT, device=d.device, dtype=torch.float64)
    w = torch.softmax(-delta * (t[None, :, None] - c[:, None, :]) ** 2, dim=2)
    live = (torch.arange(N_OUT, device=d.device)[None] < mel_len[:, None])[:, :, None]
    w = torch.where(live, w, torch.full_like(w, -1.0))
    tiles = w.view(B, -1, 64, TX // 32, 32).amax(dim=(2, 4)) if N_OUT % 64 == 0 else \
        torch.nn.functional.pad(w, (0, 0, 0, 64 - N_OUT % 64), value=-1.0).view(B, -1, 64, TX // 32, 32).amax(dim=(2, 4))
    inside = tiles >= 0
    return round(((tiles <= 2.0 ** -24) & inside).sum().item() / inside.sum().item(), 4), int(inside.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from tt2 import _lib, ops, upsample
    dev = "cuda"
    d_int = random_durations().to(dev)
    d = d_int.float()
    mel_len = d_int.sum(1).clamp(max=N_OUT).to(torch.int32)
    n_frames = int(mel_len.sum())
    center = upsample.centers(d_int).contiguous()
    prec = torch.full((B, TX), 0.1, device=dev)
    delta_t = prec.clone()
    fns, nbytes, flop, agree, peak = {}, {}, {}, {}, {}
    for name, dtype in SHAPES:
        g = torch.Generator().manual_seed(1)
        h = torch.randn(B, TX, D, generator=g).to(dev, dtype)
        dy = torch.randn(B, N_OUT, D, generator=g).to(dev, dtype)
        y, lse = torch.empty(B, N_OUT, D, dtype=dtype, device=dev), torch.empty(B, N_OUT, device=dev)
        dh, dc, dp = torch.empty_like(h), torch.empty_like(center), torch.empty_like(center)
        es = h.element_size()
        fns[f"fwd_{name}"] = lambda h=h, y=y, lse=lse: ops.gauss_upsample_fwd(h, center, prec, y, lse, q_len=mel_len)
        fns[f"bwd_{name}"] = lambda h=h, y=y, lse=lse, dy=dy, dh=dh, dc=dc, dp=dp: ops.gauss_upsample_bwd(
            h, center, prec, y, lse, dy, dh=dh, dcenter=dc, dprec=dp, q_len=mel_len)
        fns[f"bwd_dh_{name}"] = lambda h=h, y=y, lse=lse, dy=dy, dh=dh: ops.gauss_upsample_bwd(
            h, center, prec, y, lse, dy, dh=dh, q_len=mel_len)
        nbytes[f"fwd_{name}"] = es * D * (B * TX + B * N_OUT) + 4 * (B * N_OUT + 2 * B * TX)
        nbytes[f"bwd_{name}"] = es * D * (2 * B * TX + 2 * n_frames) + 4 * (n_frames + 4 * B * TX)
        nbytes[f"bwd_dh_{name}"] = es * D * (B * TX + n_frames) + 4 * (n_frames + 2 * B * TX)
        flop[f"fwd_{name}"] = 2.0 * n_frames * TX * D
        flop[f"bwd_{name}"] = 4.0 * n_frames * TX * D
        flop[f"bwd_dh_{name}"] = 2.0 * n_frames * TX * D

        def leaves(h=h):
            return h.detach().requires_grad_(), d.detach().requires_grad_(), delta_t.detach().requires_grad_()

        def whole(dy=dy):
            hh, dd, de = leaves()
            upsample.gaussian_upsample(hh, dd, mel_len=mel_len, max_frames=N_OUT, delta=de).out.backward(dy)
            return hh.grad, dd.grad, de.grad

        def torch_form(dy=dy):
            hh, dd, de = leaves()
            composed(hh, dd, mel_len, N_OUT, de).backward(dy)
            return hh.grad, dd.grad, de.grad

        def espnet_form(dy=dy):
            hh, dd, de = leaves()
            composed(hh, dd, None, N_OUT, de).backward(dy)
            return hh.grad, dd.grad, de.grad

        fns[f"whole_{name}"], fns[f"torch_{name}"], fns[f"espnet_{name}"] = whole, torch_form, espnet_form
        # the same values first
        fns[f"fwd_{name}"]()
        y_t = composed(h, d, mel_len, N_OUT, delta_t)
        ours, theirs = whole(), torch_form()
        rel = lambda x, r: round(((x.double() - r.double()).norm() / r.double().norm()).item(), 8)     # noqa: E731
        agree[name] = {"y": rel(y, y_t), "dh": rel(ours[0], theirs[0]), "d_durations": rel(ours[1], theirs[1]),
                       "d_delta": rel(ours[2], theirs[2]),
                       "ours_equal_bits_4_runs": all(all(bool(torch.equal(p, q)) for p, q in zip(whole(), ours)) for _ in range(4))}
        for leg in ("whole", "torch", "espnet"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fns[f"{leg}_{name}"]()
            torch.cuda.synchronize()
            peak[f"{leg}_{name}"] = torch.cuda.max_memory_allocated() - base
        # the fused backward's workspace sits in ops' persistent buffer, allocated before `base` was read
        workspace = int(_lib.lib().tt2_gauss_upsample_bwd_workspace_size(B, TX, N_OUT, D))
        peak[f"whole_{name}"] += workspace
    share, tiles = empty_tile_share(d_int, mel_len)
    kernel_legs = [k for k in fns if k.startswith(("fwd_", "bwd_"))]
    eager_legs = [k for k in fns if k.startswith(("whole_", "torch_", "espnet_"))]
    all_us, evi_us = timed_rounds(fns, a.rounds, torch.zeros(1 << 28, device=dev), eager=eager_legs, eager_runs=100)
    best = {k: min(v) for k, v in all_us.items()}
    evi = {k: min(v) for k, v in evi_us.items()}
    derived = {}
    for name, _ in SHAPES:
        peak_tf = BF16_MFMA_TFLOPS if name == "bf16" else F32_TFLOPS
        derived[name] = {"torch_over_whole_eager": round(best[f"torch_{name}"] / best[f"whole_{name}"], 2),
                         "torch_over_whole_evicted": round(evi[f"torch_{name}"] / evi[f"whole_{name}"], 2),
                         "espnet_over_whole_eager": round(best[f"espnet_{name}"] / best[f"whole_{name}"], 2),
                         "espnet_over_whole_evicted": round(evi[f"espnet_{name}"] / evi[f"whole_{name}"], 2),
                         "peak_bytes_torch_over_whole": round(peak[f"torch_{name}"] / max(peak[f"whole_{name}"], 1), 2),
                         "peak_bytes_espnet_over_whole": round(peak[f"espnet_{name}"] / max(peak[f"whole_{name}"], 1), 2)}
        for leg in ("fwd", "bwd", "bwd_dh"):
            k = f"{leg}_{name}"
            derived[name][f"{leg}_x_hbm_floor_evicted"] = round(evi[k] / (nbytes[k] / (HBM_GBPS * 1e3)), 1)
            derived[name][f"{leg}_tflops_resident"] = round(flop[k] / (best[k] * 1e6), 1)
            derived[name][f"{leg}_share_of_matrix_peak"] = round(flop[k] / (best[k] * 1e6) / peak_tf, 4)
    line = json.dumps({
        "shape": dict(B=B, Tx=TX, n_out=N_OUT, D=D, frames=n_frames), "agree": agree, "rounds": a.rounds, "bytes": nbytes,
        "flop": flop, "peak_bytes": peak, "workspace_bytes": workspace, "tiles_inside": tiles, "tiles_without_weight_above_2^-24": share,
        "resident_us_best": {k: round(best[k], 2) for k in kernel_legs},
        "resident_us_median": {k: round(statistics.median(all_us[k]), 2) for k in kernel_legs},
        "eager_us_best": {k: round(best[k], 2) for k in eager_legs},
        "evicted_us_best": {k: round(v, 2) for k, v in evi.items()},
        "derived": derived})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
