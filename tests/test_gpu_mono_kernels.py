"""Monotonic alignment search kernel (tt2_align_monotonic) against the numpy references of
tests/_mas_refs.py (GPU).

Exact problem: Q and K entries are integers in [-2, 2], so |s| <= 256, every path sum stays below
2^24 and every f32 operation is exact in any accumulation order: path and durations must equal
the int64 reference bit for bit (such inputs are full of ties, so the tie rule is covered).

Random problem: the path must be valid and its float64 score within the derived f32 rounding
bound of the optimum, F(pi*) - F(pi_gpu) <= 1.01 * 2 Ty (delta + u M), u = 2^-24,
delta = 64 u max_{n,t} sum_d |q_nd k_td| (a 64-term f32 dot), M = sum_n max_t |s64[n, t]| (one
rounded add per row on sums no greater than M): either path's f32 value is within Ty (delta + u M)
of its float64 value.

Peaky problem: q_n += 2 k_floor(n Tx / Ty); the per-row argmax path is then itself monotone (that
is asserted on the CPU first, with a top-2 gap >= 1e-4 on every row), so the search must return
tt2_attn_align's amax and tt2_align_durations' histogram.

logp: distance to the float64 value along the returned path, bar max(2e-6, 2 x the distance of a
plain float32 CPU evaluation from float64) (test_gpu_align_kernels.py's rule); the test prints
floor and value before it asserts.  The distance is absolute (the greatest over the utterances):
logp is a difference of O(10) terms (score - LSE) that comes arbitrarily close to 0 on a sharp
alignment (-5e-4 on the peaky problem), so a relative measure would be ill-conditioned there, and
on the random problem (logp about -5) the absolute bar is the stricter of the two.

Measured (MI355X): the random problems' paths equal the float64 optimum on every frame (gap 0
against bounds of 4e-2 .. 1.1); logp errors 5e-8 .. 4.6e-7 against floors of 1e-8 .. 6.2e-7, so
the bar in force is 2e-6 everywhere.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _mas_refs import check_path, durations_of, mas_path, path_score  # noqa: E402
from tt2 import _lib, ops  # noqa: E402

D = 64
H = 2
L = 2          # layer slots
HD = H * D
SCALE = 1.0 / math.sqrt(D)
GUARD = 64
RUNS = [(torch.bfloat16, 0), (torch.bfloat16, 1), (torch.float32, 0)]
RUN_IDS = ["bf16-0", "bf16-1", "f32-0"]

# Tq, Tk, q_len, key_len, sel (layer slot, head) per utterance
EXACT = [
    # 32-row block edge x 64-key tile edge; Tx_b = 1; q_len = 0; out-of-range sel entries
    (31, 63, [31, 20, 0, 31, 31], [63, 1, 40, 63, 63], [(0, 0), (1, 1), (0, 1), (2, 0), (0, H)]),
    (32, 64, [32, 32, 5, 32], [64, 32, 0, 7], [(1, 0), (0, 1), (0, 0), (1, 1)]),   # Ty = Tx; key_len = 0
    (33, 65, [33, 10, 33], [65, 33, 64], [(0, 1), (1, 0), (1, 1)]),                # Ty < Tx
    (65, 129, None, None, [(1, 1), (0, 0)]),                                       # no length vectors
    # move-word boundaries
    (40, 31, [40, 33], [31, 30], [(0, 0), (1, 1)]),
    (40, 32, [40, 32], [32, 31], [(1, 0), (0, 1)]),
    (40, 33, [40, 33], [33, 32], [(0, 1), (1, 0)]),
    # every lane's key run at the largest tk
    (_lib.MONO_MAX_KEYS + 8, _lib.MONO_MAX_KEYS, [_lib.MONO_MAX_KEYS + 8, _lib.MONO_MAX_KEYS],
     [_lib.MONO_MAX_KEYS, _lib.MONO_MAX_KEYS - 1], [(0, 1), (1, 0)]),
    # the 512-key capacity with the move bits in LDS (at most 256 frames; the case above and
    # test_move_bits_in_the_workspace hold the two capacities whose bits go to the workspace)
    (40, 300, [40, 33], [300, 270], [(0, 1), (1, 0)]),
]
REAL = [
    (65, 129, None, None, [(1, 1), (0, 0)]),
    (131, 133, [131, 90, 70], [133, 70, 70], [(0, 0), (1, 1), (1, 0)]),
    (200, 96, [200, 123], [96, 50], [(1, 0), (0, 1)]),
    (_lib.MONO_MAX_KEYS + 8, _lib.MONO_MAX_KEYS, [_lib.MONO_MAX_KEYS + 8, 300], [_lib.MONO_MAX_KEYS, 257],
     [(0, 1), (1, 0)]),
]


def guarded(n, dtype):
    """A [n] tensor of `dtype` (4 bytes) inside a NaN-filled f32 buffer: (whole, interior)."""
    whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(dtype)


def guards_intact(whole, n):
    return bool(torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + n:]).all())


class Problem:
    """L layer slots of Q, K (column slices of one wide buffer, as the engine's mkv) and forward LSE."""

    def __init__(self, case, kind, dtype, seed=0):
        Tq, Tk, ql, kl, sel = case
        B = len(sel)
        self.case, self.dtype, self.B, self.Tq, self.Tk, self.sel = case, dtype, B, Tq, Tk, sel
        self.ty = [Tq] * B if ql is None else [min(max(x, 0), Tq) for x in ql]
        self.tx = [Tk] * B if kl is None else [min(max(x, 0), Tk) for x in kl]
        g = torch.Generator().manual_seed(1000 * seed + 7 * Tq + Tk)
        if kind == "exact":
            qs = [torch.randint(-2, 3, (B, Tq, HD), generator=g).float() for _ in range(L)]
            wide = torch.randint(-2, 3, (B, Tk, L * 2 * HD), generator=g).float()
        else:
            qs = [torch.randn(B, Tq, HD, generator=g) for _ in range(L)]
            wide = torch.randn(B, Tk, L * 2 * HD, generator=g)
            if kind == "peaky":
                for l in range(L):
                    for b in range(B):
                        n = torch.arange(self.ty[b])
                        qs[l][b, :self.ty[b]] += 2 * wide[b, (n * self.tx[b]) // max(self.ty[b], 1),
                                                          2 * HD * l:2 * HD * l + HD]
        self.q_d = [q.reshape(B * Tq, HD).to(dtype).cuda() for q in qs]
        self.wide_d = wide.reshape(B * Tk, L * 2 * HD).to(dtype).cuda()
        self.k_d = [self.wide_d[:, 2 * HD * l:] for l in range(L)]
        self.klen_d = None if kl is None else torch.tensor(kl, dtype=torch.int32).cuda()
        self.qlen_d = None if ql is None else torch.tensor(ql, dtype=torch.int32).cuda()
        self.sel_d = torch.tensor(sel, dtype=torch.int32).cuda()
        self.lse = []
        for l in range(L):
            out = torch.zeros(B * Tq, HD, dtype=dtype, device="cuda")
            lse = torch.zeros(B * H, Tq, dtype=torch.float32, device="cuda")
            ops.attn_fwd(self.q_d[l], self.k_d[l], self.wide_d[:, 2 * HD * l + HD:], out, lse, HD, L * 2 * HD,
                         L * 2 * HD, HD, B, H, Tq, Tk, self.klen_d, False, SCALE)
            self.lse.append(lse)
        # the inputs as the kernel sees them (rounded to dtype), in float64
        self.q64 = [q.to(dtype).double().view(B, Tq, H, D) for q in qs]
        self.k64 = [wide.to(dtype).double()[:, :, 2 * HD * l:2 * HD * l + HD].reshape(B, Tk, H, D) for l in range(L)]

    def valid(self, b):
        li, h = self.sel[b]
        return self.ty[b] > 0 and self.tx[b] > 0 and 0 <= li < L and 0 <= h < H

    def qk(self, b):
        li, h = self.sel[b]
        return self.q64[li][b, :, h], self.k64[li][b, :, h]

    def scores(self, b):
        q, k = self.qk(b)
        return (q @ k.T).numpy()

    def run(self, variant, sel=True, head=None):
        B, Tq, Tk = self.B, self.Tq, self.Tk
        bufs = [guarded(B * Tq, torch.int32), guarded(B * Tk, torch.int32), guarded(B, torch.float32)]
        ops.align_monotonic(self.q_d, self.k_d, self.lse, bufs[0][1], bufs[1][1], bufs[2][1], HD, L * 2 * HD, B, H,
                            Tq, Tk, key_len=self.klen_d, q_len=self.qlen_d, sel=self.sel_d if sel else None,
                            head=head, scale=SCALE, variant=variant)
        torch.cuda.synchronize()
        for (whole, _), n in zip(bufs, (B * Tq, B * Tk, B)):
            assert guards_intact(whole, n)
        return (bufs[0][1].view(B, Tq).cpu().numpy().astype(np.int64),
                bufs[1][1].view(B, Tk).cpu().numpy().astype(np.int64), bufs[2][1].cpu())

    def logp_refs(self, b, path):
        """mean ln P[n, path[n]] in float64 and in a plain float32 evaluation."""
        q, k = self.qk(b)
        ty, tx = self.ty[b], self.tx[b]
        idx = torch.as_tensor(path[:ty]).view(-1, 1)
        out = []
        for dt in (torch.float64, torch.float32):
            s = (q[:ty].to(dt) @ k[:tx].to(dt).T) * SCALE
            out.append(float(torch.log_softmax(s, -1).gather(1, idx).mean()))
        return out

    def check_logp(self, logp, path, tag):
        want, f32 = [], []
        rows = [b for b in range(self.B) if self.valid(b)]
        for b in rows:
            w, f = self.logp_refs(b, path[b])
            want.append(w)
            f32.append(f)
        want, f32, got = np.array(want), np.array(f32), logp.double().numpy()[rows]
        floor, err = np.abs(f32 - want).max(), np.abs(got - want).max()
        bar = max(2e-6, 2 * floor)
        print(f"{tag}: logp {want.min():.4f}..{want.max():.4f} abs err {err:.3e} floor {floor:.3e} bar {bar:.3e}")
        assert err <= bar, (err, bar)


_problems = {}


def problem(cases, ci, kind, dtype):
    key = (ci, kind, dtype)
    if key not in _problems:
        _problems[key] = Problem(cases[ci], kind, dtype)
    return _problems[key]


def check_shape_of_outputs(P, path, dur, logp):
    """What holds for every problem: invalid utterances, tails, sums."""
    for b in range(P.B):
        ty, tx = P.ty[b], P.tx[b]
        if not P.valid(b):
            assert (path[b] == -1).all() and (dur[b] == 0).all() and float(logp[b]) == 0.0, b
            continue
        assert check_path(path[b, :ty], ty, tx) is None, (b, check_path(path[b, :ty], ty, tx))
        assert (path[b, ty:] == -1).all(), b
        assert np.array_equal(dur[b], durations_of(path[b, :ty], P.Tk)), b
        assert dur[b].sum() == ty and (dur[b, min(tx, ty):] == 0).all()
        if ty >= tx:
            assert (dur[b, :tx] >= 1).all()


@pytest.mark.parametrize("dtype,variant", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("ci", range(len(EXACT)))
def test_exact_problem_bit_for_bit(ci, dtype, variant):
    P = problem(EXACT, ci, "exact", dtype)
    path, dur, logp = P.run(variant)
    check_shape_of_outputs(P, path, dur, logp)
    for b in range(P.B):
        if P.valid(b):
            s = P.scores(b)
            assert np.array_equal(s, np.rint(s)) and np.abs(s).max() <= 256
            want = mas_path(s.astype(np.int64), P.ty[b], P.tx[b])
            assert np.array_equal(path[b, :P.ty[b]], want), (b, path[b, :P.ty[b]], want)
            assert np.array_equal(dur[b], durations_of(want, P.Tk)), b


@pytest.mark.parametrize("dtype,variant", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("ci", range(len(REAL)))
def test_random_problem_within_the_rounding_bound(ci, dtype, variant):
    P = problem(REAL, ci, "randn", dtype)
    path, dur, logp = P.run(variant)
    check_shape_of_outputs(P, path, dur, logp)
    u = 2.0 ** -24
    for b in range(P.B):
        if not P.valid(b):
            continue
        ty, tx = P.ty[b], P.tx[b]
        q, k = P.qk(b)
        s = P.scores(b)[:ty, :tx]
        best = mas_path(s, ty, tx)
        gap = path_score(s, best) - path_score(s, path[b, :ty])
        delta = 64 * u * float((q[:ty].abs() @ k[:tx].abs().T).max())
        M = float(np.abs(s).max(1).sum())
        bound = 1.01 * 2 * ty * (delta + u * M)
        print(f"case {ci} {RUN_IDS[RUNS.index((dtype, variant))]} b {b}: F(pi*) - F(pi_gpu) = {gap:.3e}, bound {bound:.3e}, "
              f"{int((best != path[b, :ty]).sum())} frames differ")
        assert -1e-9 <= gap <= bound, (gap, bound)
    P.check_logp(logp, path, f"randn case {ci}")
    again = P.run(variant)
    assert np.array_equal(path, again[0]) and np.array_equal(dur, again[1])
    assert torch.equal(logp.view(torch.int32), again[2].view(torch.int32))   # bit-identical run to run


PEAKY = [
    (65, 33, None, None, [(1, 1), (1, 1)]),
    (131, 133, [131, 90, 70], [120, 70, 1], [(0, 1), (0, 1), (0, 1)]),
    (200, 96, [200, 123], [96, 50], [(1, 0), (1, 0)]),
]


@pytest.mark.parametrize("dtype,variant", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("ci", range(len(PEAKY)))
def test_peaky_problem_equals_the_argmax_path(ci, dtype, variant):
    P = problem(PEAKY, ci, "peaky", dtype)
    li, h = P.sel[0]
    # CPU, float64 only: the per-row argmax path is a valid monotone path with a clear gap
    for b in range(P.B):
        ty, tx = P.ty[b], P.tx[b]
        s = torch.from_numpy(P.scores(b)[:ty, :tx]) * SCALE
        am = s.argmax(-1).numpy()
        assert check_path(am, ty, tx) is None, (b, check_path(am, ty, tx))
        if tx > 1:
            top = s.topk(2, dim=-1).values
            assert float((top[:, 0] - top[:, 1]).min()) >= 1e-4
    path, dur, logp = P.run(variant, sel=False, head=(li, h))
    check_shape_of_outputs(P, path, dur, logp)
    B, Tq, Tk = P.B, P.Tq, P.Tk
    pmax = torch.zeros(L, B * H, Tq, dtype=torch.float32, device="cuda")
    amax = torch.zeros(L, B * H, Tq, dtype=torch.int32, device="cuda")
    ops.attn_align(P.q_d, P.k_d, P.lse, pmax, amax, HD, L * 2 * HD, B, H, Tq, Tk, key_len=P.klen_d, q_len=P.qlen_d,
                   scale=SCALE, variant=variant)
    focus = torch.zeros(L, B, H, device="cuda")
    sel = torch.zeros(B, 2, dtype=torch.int32, device="cuda")
    sf = torch.zeros(B, device="cuda")
    d2 = torch.zeros(B, Tk, dtype=torch.int32, device="cuda")
    ops.align_durations(pmax, amax, focus, sel, sf, d2, L, B, H, Tq, Tk, key_len=P.klen_d, q_len=P.qlen_d,
                        head=(li, h))
    assert np.array_equal(path, amax.view(L, B, H, Tq)[li, :, h].cpu().numpy())
    assert np.array_equal(dur, d2.cpu().numpy())
    # the same through sel, as tt2_align_durations wrote it
    p2 = guarded(B * Tq, torch.int32)[1]
    d3 = guarded(B * Tk, torch.int32)[1]
    l3 = guarded(B, torch.float32)[1]
    ops.align_monotonic(P.q_d, P.k_d, P.lse, p2, d3, l3, HD, L * 2 * HD, B, H, Tq, Tk, key_len=P.klen_d,
                        q_len=P.qlen_d, sel=sel, scale=SCALE, variant=variant)
    assert np.array_equal(p2.view(B, Tq).cpu().numpy(), path) and torch.equal(l3.cpu(), logp)
    P.check_logp(logp, path, f"peaky case {ci}")


def test_wrapper_and_library_refuse_bad_requests():
    P = problem(EXACT, 4, "exact", torch.bfloat16)
    B, Tq, Tk = P.B, P.Tq, P.Tk
    path = torch.zeros(B * Tq, dtype=torch.int32, device="cuda")
    dur = torch.zeros(B * Tk, dtype=torch.int32, device="cuda")
    logp = torch.zeros(B, device="cuda")
    args = (P.q_d, P.k_d, P.lse)
    tail = (HD, L * 2 * HD, B, H, Tq, Tk)
    big = _lib.MONO_MAX_KEYS + 1
    kbig = [torch.zeros(B * big, L * 2 * HD, dtype=torch.bfloat16, device="cuda")] * L
    dbig = torch.zeros(B * big, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.TT2Error, match="TT2_MONO_MAX_KEYS"):
        ops.align_monotonic(P.q_d, kbig, P.lse, path, dbig, logp, HD, L * 2 * HD, B, H, Tq, big, head=(0, 0))
    with pytest.raises(_lib.TT2Error, match="path"):
        ops.align_monotonic(*args, path[:-1], dur, logp, *tail, head=(0, 0))
    with pytest.raises(_lib.TT2Error, match="durations"):
        ops.align_monotonic(*args, path, dur.float(), logp, *tail, head=(0, 0))
    with pytest.raises(_lib.TT2Error, match="logp"):
        ops.align_monotonic(*args, path, dur, logp[:-1], *tail, head=(0, 0))
    with pytest.raises(_lib.TT2Error, match="sel"):
        ops.align_monotonic(*args, path, dur, logp, *tail, sel=P.sel_d.long())
    with pytest.raises(_lib.TT2Error, match="either sel or head"):
        ops.align_monotonic(*args, path, dur, logp, *tail)
    with pytest.raises(_lib.TT2Error, match="fixed head"):
        ops.align_monotonic(*args, path, dur, logp, *tail, head=(L, 0))
    with pytest.raises(_lib.TT2Error, match="variant"):
        ops.align_monotonic(*args, path, dur, logp, *tail, head=(0, 0), variant=2)
    with pytest.raises(_lib.TT2Error, match="scale"):
        ops.align_monotonic(*args, path, dur, logp, *tail, head=(0, 0), scale=0.0)


def test_move_bits_in_the_workspace():
    """256-key capacity keeps the move bits of at most 1536 frames in LDS: at 1600 frames they go
    to the workspace.  The exact problem again, bit for bit."""
    Tq, Tk = 1600, 200
    assert _lib.load().tt2_align_monotonic_workspace_size(2, Tq, Tk) > 0
    case = (Tq, Tk, [1600, 1550], [200, 129], [(0, 1), (1, 0)])
    P = Problem(case, "exact", torch.bfloat16)
    path, dur, logp = P.run(0)
    check_shape_of_outputs(P, path, dur, logp)
    for b in range(P.B):
        want = mas_path(P.scores(b).astype(np.int64), P.ty[b], P.tx[b])
        assert np.array_equal(path[b, :P.ty[b]], want), b
