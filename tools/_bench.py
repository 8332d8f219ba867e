"""What the data-path bench tools (pitch, pitch_track, dtw, resample, trim, loudness, regulate) share:
tests/ and the package on sys.path, the test signal, and the timing legs over gemm_ab's graph_of /
time_graph.  "Resident" is ten back-to-back runs in a replayed hipGraph, "evicted" single runs between
device events after a 1 GiB buffer has been rewritten, "eager" back-to-back calls between device
events (host time included)."""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gemm_ab import graph_of, time_graph  # noqa: E402

HBM_GBPS = 6290.0     # measured float4 copy rate of one MI355X (the guide's figure)


def speech_like(B, L, seed=0):
    """Voiced stretches with a gliding pitch and three harmonics, noisy stretches between them."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / 22050.0
    out = torch.zeros(B, L, dtype=torch.float64)
    for b in range(B):
        f = 90.0 + 20.0 * b + 30.0 * torch.sin(2 * math.pi * (0.7 + 0.05 * b) * t)
        ph = 2 * math.pi * torch.cumsum(f, 0) / 22050.0
        tone = 0.3 * torch.sin(ph) + 0.15 * torch.sin(2 * ph + 0.5) + 0.08 * torch.sin(3 * ph + 1.1)
        voiced = (torch.sin(2 * math.pi * 1.3 * t + b) > -0.3).double()
        out[b] = tone * voiced + (0.01 + 0.1 * (1 - voiced)) * torch.randn(L, generator=g, dtype=torch.float64)
    return out.float()


def evicted_us(fn, trash, reps):
    out = []
    for _ in range(reps):
        trash.add_(1.0)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        fn()
        e[1].record()
        torch.cuda.synchronize()
        out.append(e[0].elapsed_time(e[1]) * 1e3)
    return min(out)


def eager_us(fn, n):
    """us per run of n back-to-back eager runs (launch overhead included)."""
    fn()
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    for _ in range(n):
        fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]) * 1e3 / n


def wall_us(fn):
    """Host wall time of one run, synchronised either side."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def timed_rounds(fns, rounds, trash, eager=(), eager_runs=10, each_round=None):
    """(resident_us, evicted_us): per leg of fns (name -> callable) one figure per round.  The legs
    named in `eager` are not captured: their resident figure is eager_us over eager_runs runs.
    each_round() runs at the end of every round (a baseline timed some other way)."""
    graphs = {k: graph_of(f) for k, f in fns.items() if k not in eager}
    res_us = {k: [] for k in fns}
    evi_us = {k: [] for k in fns}
    for _ in range(rounds):   # interleaved: drift of the machine hits every path alike
        for k in fns:
            res_us[k].append(time_graph(graphs[k]) * 1e6 if k in graphs else eager_us(fns[k], eager_runs))
            evi_us[k].append(evicted_us(fns[k], trash, 3))
        if each_round is not None:
            each_round()
    return res_us, evi_us
