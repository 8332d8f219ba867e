"""Alignment-statistics kernels (tt2_attn_align / tt2_align_durations) vs a float64 torch
reference computed from the inputs after rounding to the test dtype (GPU).

amax: equal to the reference argmax on every valid row whose reference top-2 gap in scaled score
is >= 1e-4 (about 100x the f32 rounding of a 64-term dot at these magnitudes); on rows under that
gap one of the reference's top two; such rows are at most 0.5 % of the valid rows.

pmax (relative Frobenius norm over all rows): the bar is not fixed in advance.
  f32:  max(2e-6, 2 x the distance of a plain float32 CPU evaluation of the reference from the
        float64 one)  -- test_gpu_guided_attention.py's rule;
  bf16: max(2e-6, 2 x the distance of the path this replaces, tt2_attn_probs -> amax(-1), from the
        same reference, run in the same test).
Measured floors (the test prints them before it asserts; MI355X, the ten problems below):
  f32 CPU evaluation vs float64: 1.2e-7 .. 3.3e-7 (0 with a single key)
  tt2_attn_probs -> amax, bf16:  5.4e-8 .. 6.7e-7
so the bar in force is 2e-6 everywhere.  Measured against it: f32 1.7e-7 .. 1.2e-6, bf16 plain
kernel (variant 1) 5.9e-8 .. 6.9e-7, bf16 MFMA kernels (variants 0, 2, 3) 1.6e-8 .. 2.6e-7.  No row
of these problems falls under the top-2 gap.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tt2 import _lib, ops  # noqa: E402

D = 64
GAP = 1e-4

CASES = [
    # B, H, Tq, Tk, key_len, q_len
    (3, 3, 131, 133, [133, 70, 0], [131, 40, 17]),   # tails on both axes; an empty utterance
    (2, 2, 70, 37, [37, 20], [70, 0]),               # Tk < 64; an utterance with no valid row
    (1, 8, 64, 128, None, None),                     # no length vectors
    (2, 8, 200, 96, [96, 50], [200, 123]),
    (1, 2, 33, 1, None, None),                       # a single key
]
KINDS = ["randn", "peaky"]
RUNS = [(torch.float32, 0)] + [(torch.bfloat16, v) for v in (0, 1, 2, 3)]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def lens_of(case):
    B, H, Tq, Tk, kl, ql = case
    tx = torch.full((B,), Tk) if kl is None else torch.tensor(kl).clamp(max=Tk)
    ty = torch.full((B,), Tq) if ql is None else torch.tensor(ql).clamp(max=Tq)
    return tx, ty


def ref_stats(q, k, tx, ty, scale):
    """q [B,H,Tq,64], k [B,H,Tk,64] in the evaluation dtype.  Returns pmax [B,H,Tq] (0 on invalid
    rows), the top-2 scaled scores' key indices [B,H,Tq,2], their gap and the validity mask."""
    B, H, Tq, _ = q.shape
    Tk = k.shape[2]
    s = (q @ k.transpose(-1, -2)) * scale
    vis = (torch.arange(Tk)[None, :] < tx[:, None]).view(B, 1, 1, Tk)
    s = s.masked_fill(~vis, float("-inf"))
    valid = ((torch.arange(Tq)[None, :] < ty[:, None]) & (tx[:, None] > 0)).view(B, 1, Tq).expand(B, H, Tq)
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(s - mx) * vis
    den = e.sum(-1)
    pmax = torch.where(valid, 1.0 / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    top = s.topk(min(2, Tk), dim=-1)
    idx = top.indices if Tk > 1 else torch.cat([top.indices, top.indices], -1)
    gap = (top.values[..., 0] - top.values[..., 1]) if Tk > 1 else torch.full_like(den, float("inf"))
    gap = torch.where(torch.isnan(gap), torch.full_like(gap, float("inf")), gap)   # (-inf) - (-inf)
    return pmax, idx, gap, valid


class Problem:
    """One (case, kind, dtype): device tensors, the forward's LSE and the float64 reference."""

    def __init__(self, case, kind, dtype):
        B, H, Tq, Tk, kl, ql = case
        self.case, self.dtype = case, dtype
        self.scale = 1.0 / math.sqrt(D)
        HD = self.HD = H * D
        g = torch.Generator().manual_seed(B * 100 + Tq + Tk)
        q = torch.randn(B * Tq, HD, generator=g)
        kv = torch.randn(B * Tk, 2 * HD, generator=g)
        self.tx, self.ty = tx, ty = lens_of(case)
        if kind == "peaky":   # query n looks at key floor(n * Tx_b / Ty_b)
            q3, k3 = q.view(B, Tq, HD), kv.view(B, Tk, 2 * HD)[:, :, :HD]
            for b in range(B):
                if tx[b] > 0 and ty[b] > 0:
                    n = torch.arange(int(ty[b]))
                    q3[b, :int(ty[b])] += k3[b, (n * int(tx[b])) // int(ty[b])]
        self.q_d, self.kv_d = q.to(dtype).cuda(), kv.to(dtype).cuda()
        self.klen_d = None if kl is None else torch.tensor(kl, dtype=torch.int32).cuda()
        self.qlen_d = None if ql is None else torch.tensor(ql, dtype=torch.int32).cuda()

        def heads(x, T):
            return x.to(dtype).double().view(B, T, H, D).transpose(1, 2)

        qr, kr = heads(q, Tq), heads(kv[:, :HD], Tk)
        self.pmax_ref, self.top2, self.gap, self.valid = ref_stats(qr, kr, tx, ty, self.scale)
        p32 = ref_stats(qr.float(), kr.float(), tx, ty, self.scale)[0]
        self.floor32 = rel(p32, self.pmax_ref)
        # the forward's LSE (and the probabilities path this replaces)
        out = torch.zeros(B * Tq, HD, dtype=dtype, device="cuda")
        self.lse = torch.zeros(B * H, Tq, dtype=torch.float32, device="cuda")
        ops.attn_fwd(self.q_d, self.kv_d[:, :HD], self.kv_d[:, HD:], out, self.lse, HD, 2 * HD, 2 * HD, HD, B, H, Tq,
                     Tk, self.klen_d, False, self.scale)
        self._old = None

    def old_path(self):
        """tt2_attn_probs -> amax(-1), zeroed past q_len as the new kernel's rows are."""
        if self._old is None:
            B, H, Tq, Tk, _, _ = self.case
            probs = torch.zeros(B * H, Tq, Tk, dtype=torch.float32, device="cuda")
            ops.attn_probs(self.q_d, self.kv_d[:, :self.HD], self.lse, probs, self.HD, 2 * self.HD, B, H, Tq, Tk,
                           key_len=self.klen_d, scale=self.scale)
            self._old = probs.amax(-1).view(B, H, Tq).cpu() * self.valid
        return self._old

    def align(self, variant, q=None, k=None, lse=None, k_ld=None):
        B, H, Tq, Tk, _, _ = self.case
        qs = [self.q_d] if q is None else q
        ks = [self.kv_d[:, :self.HD]] if k is None else k
        ls = [self.lse] if lse is None else lse
        n = len(qs)
        pmax = torch.full((n, B * H, Tq), 7.0, dtype=torch.float32, device="cuda")
        amax = torch.full((n, B * H, Tq), 77, dtype=torch.int32, device="cuda")
        ops.attn_align(qs, ks, ls, pmax, amax, self.HD, 2 * self.HD if k_ld is None else k_ld, B, H, Tq, Tk,
                       key_len=self.klen_d, q_len=self.qlen_d, scale=self.scale, variant=variant)
        return pmax.view(n, B, H, Tq), amax.view(n, B, H, Tq)


_problems = {}


def problem(ci, kind, dtype):
    key = (ci, kind, dtype)
    if key not in _problems:
        _problems[key] = Problem(CASES[ci], kind, dtype)
    return _problems[key]


@pytest.mark.parametrize("dtype,variant", RUNS, ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_align_vs_float64(ci, kind, dtype, variant):
    P = problem(ci, kind, dtype)
    pmax, amax = P.align(variant)
    pmax, amax = pmax[0].cpu(), amax[0].cpu().long()
    valid = P.valid
    # invalid rows: exactly 0 and -1
    assert (pmax[~valid] == 0).all() and (amax[~valid] == -1).all()
    assert (pmax <= 1 + 1e-5).all(), pmax.max().item()
    nvalid = int(valid.sum())
    if nvalid:
        a, top2, gap = amax[valid], P.top2[valid], P.gap[valid]
        clear = gap >= GAP
        assert (a[clear] == top2[clear][:, 0]).all(), "argmax differs on a row with a clear top-2 gap"
        assert ((a[~clear] == top2[~clear][:, 0]) | (a[~clear] == top2[~clear][:, 1])).all()
        assert int((~clear).sum()) <= 0.005 * nvalid, (int((~clear).sum()), nvalid)
    if P.pmax_ref.norm() == 0:
        assert (pmax == 0).all()
        return
    err = rel(pmax, P.pmax_ref)
    if dtype == torch.float32:
        floor = P.floor32
    else:
        floor = rel(P.old_path(), P.pmax_ref)
    bar = max(2e-6, 2 * floor)
    print(f"case {ci} {kind} {dtype} variant {variant}: pmax rel {err:.3e} floor {floor:.3e} bar {bar:.3e} "
          f"rows under the gap {int((P.gap[valid] < GAP).sum())} of {nvalid}")
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("dtype,variant", RUNS, ids=lambda x: str(x).replace("torch.", ""))
def test_exact_ties_take_the_lowest_index(dtype, variant):
    """Keys 9, 13 and 69 are copies of key 5 (the other half of the lane pair, the same lane, the
    next key tile) and every query points at it: amax is 5."""
    B, H, Tq, Tk = 2, 2, 70, 133
    HD = H * D
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, Tq, HD, generator=g) * 0.1
    kv = torch.randn(B, Tk, 2 * HD, generator=g)
    for t in (9, 13, 69):
        kv[:, t] = kv[:, 5]
    q += kv[:, 5:6, :HD]
    q_d, kv_d = q.view(B * Tq, HD).to(dtype).cuda(), kv.view(B * Tk, 2 * HD).to(dtype).cuda()
    out = torch.zeros(B * Tq, HD, dtype=dtype, device="cuda")
    lse = torch.zeros(B * H, Tq, dtype=torch.float32, device="cuda")
    ops.attn_fwd(q_d, kv_d[:, :HD], kv_d[:, HD:], out, lse, HD, 2 * HD, 2 * HD, HD, B, H, Tq, Tk, None, False, 0.125)
    pmax = torch.zeros(1, B * H, Tq, dtype=torch.float32, device="cuda")
    amax = torch.zeros(1, B * H, Tq, dtype=torch.int32, device="cuda")
    ops.attn_align([q_d], [kv_d[:, :HD]], [lse], pmax, amax, HD, 2 * HD, B, H, Tq, Tk, scale=0.125, variant=variant)
    assert (amax == 5).all(), amax.unique().tolist()
    # four equal maxima share the row: each holds a quarter of (almost) all the weight
    assert (pmax <= 0.25 + 1e-5).all() and (pmax > 0.2).all()


@pytest.mark.parametrize("dtype,variant", [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1),
                                           (torch.bfloat16, 3)], ids=lambda x: str(x).replace("torch.", ""))
def test_multi_layer_launch_equals_single_launches(dtype, variant):
    """L = 3: distinct Q and LSE per layer, K as column slices of one wide buffer (as mkv is)."""
    case = CASES[0]
    B, H, Tq, Tk, kl, ql = case
    HD = H * D
    L = 3
    P = problem(0, "randn", dtype)
    g = torch.Generator().manual_seed(11)
    wide = torch.randn(B * Tk, L * 2 * HD, generator=g).to(dtype).cuda()
    qs = [torch.randn(B * Tq, HD, generator=g).to(dtype).cuda() for _ in range(L)]
    ks = [wide[:, 2 * HD * l:] for l in range(L)]
    lses = []
    for l in range(L):
        out = torch.zeros(B * Tq, HD, dtype=dtype, device="cuda")
        lse = torch.zeros(B * H, Tq, dtype=torch.float32, device="cuda")
        ops.attn_fwd(qs[l], ks[l], wide[:, 2 * HD * l + HD:], out, lse, HD, L * 2 * HD, L * 2 * HD, HD, B, H, Tq, Tk,
                     P.klen_d, False, P.scale)
        lses.append(lse)
    pm, am = P.align(variant, qs, ks, lses, k_ld=L * 2 * HD)
    assert len(torch.unique(am[:, 0, 0, :17], dim=0)) == L   # the layers differ
    for l in range(L):
        p1, a1 = P.align(variant, [qs[l]], [ks[l]], [lses[l]], k_ld=L * 2 * HD)
        assert torch.equal(pm[l], p1[0]) and torch.equal(am[l], a1[0]), l


def run_durations(pm, am, case, klen_d, qlen_d, head=None):
    L, B, H, Tq = pm.shape
    Tk = case[3]
    focus = torch.full((L, B, H), 7.0, dtype=torch.float32, device="cuda")
    sel = torch.full((B, 2), 77, dtype=torch.int32, device="cuda")
    sel_focus = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    dur = torch.full((B, Tk), 77, dtype=torch.int32, device="cuda")
    ops.align_durations(pm, am, focus, sel, sel_focus, dur, L, B, H, Tq, Tk, key_len=klen_d, q_len=qlen_d, head=head)
    return focus, sel, sel_focus, dur


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_durations_vs_torch(ci, kind):
    """tt2_align_durations against torch on the kernel's own pmax / amax (two layer slots: the
    peaky / randn problem and its bf16 twin's statistics, so the heads differ)."""
    case = CASES[ci]
    B, H, Tq, Tk, _, _ = case
    P = problem(ci, kind, torch.float32)
    Pb = problem(ci, kind, torch.bfloat16)
    p0, a0 = P.align(0)
    p1, a1 = Pb.align(0)
    pm, am = torch.cat([p0, p1]).contiguous(), torch.cat([a0, a1]).contiguous()
    L = 2
    tx, ty = P.tx, P.ty
    focus, sel, sel_focus, dur = run_durations(pm, am, case, P.klen_d, P.qlen_d)
    again = run_durations(pm, am, case, P.klen_d, P.qlen_d)
    for x, y in zip((focus, sel, sel_focus, dur), again):
        assert torch.equal(x, y)   # bit-identical run to run
    pmc, amc = pm.cpu(), am.cpu().long()
    focus, sel, sel_focus, dur = focus.cpu(), sel.cpu().long(), sel_focus.cpu(), dur.cpu().long()
    for b in range(B):
        n = int(ty[b])
        want = pmc[:, b, :, :n].double().sum(-1) / max(n, 1)   # [L, H]
        assert torch.allclose(focus[:, b].double(), want, rtol=1e-6, atol=0), (b, focus[:, b], want)
        flat = int(torch.argmax(focus[:, b].reshape(-1)))   # first maximum = lowest flat index
        assert sel[b].tolist() == [flat // H, flat % H], (b, sel[b], flat)
        assert sel_focus[b] == focus[flat // H, b, flat % H]
        rows = amc[flat // H, b, flat % H, :n]
        rows = rows[rows >= 0]
        assert torch.equal(dur[b], torch.bincount(rows, minlength=Tk)), b
        assert int(dur[b].sum()) == (n if tx[b] > 0 else 0)
        assert (dur[b, int(tx[b]):] == 0).all()
    # mode 1: the given head for every utterance
    fixed = (1, H - 1)
    focus1, sel1, sel_focus1, dur1 = [x.cpu() for x in run_durations(pm, am, case, P.klen_d, P.qlen_d, head=fixed)]
    assert torch.equal(focus1, focus)
    for b in range(B):
        n = int(ty[b])
        assert sel1[b].tolist() == list(fixed)
        assert sel_focus1[b] == focus[1, b, H - 1]
        rows = amc[1, b, H - 1, :n]
        assert torch.equal(dur1[b].long(), torch.bincount(rows[rows >= 0], minlength=Tk))
        assert int(dur1[b].sum()) == (n if tx[b] > 0 else 0)


def test_best_head_tie_takes_the_lowest_flat_index():
    """Equal focus in (slot 0, head 2), (slot 1, head 0): the first wins."""
    L, B, H, Tq, Tk = 2, 2, 3, 40, 9
    pm = torch.full((L, B, H, Tq), 0.25, device="cuda")
    pm[0, :, 2] = 0.5
    pm[1, :, 0] = 0.5
    am = torch.zeros(L, B, H, Tq, dtype=torch.int32, device="cuda")
    am[0, :, 2] = 4
    focus, sel, sel_focus, dur = run_durations(pm, am, (B, H, Tq, Tk, None, None), None, None)
    assert sel.cpu().tolist() == [[0, 2], [0, 2]]
    assert (sel_focus == 0.5).all() and (dur[:, 4] == Tq).all() and int(dur.sum()) == B * Tq


def test_wrappers_refuse_bad_requests():
    P = problem(1, "randn", torch.bfloat16)
    B, H, Tq, Tk, _, _ = P.case
    HD = P.HD
    pmax = torch.zeros(1, B * H, Tq, dtype=torch.float32, device="cuda")
    amax = torch.zeros(1, B * H, Tq, dtype=torch.int32, device="cuda")
    args = ([P.q_d], [P.kv_d[:, :HD]], [P.lse])
    tail = (HD, 2 * HD, B, H, Tq, Tk)
    with pytest.raises(_lib.TT2Error, match="causal"):
        ops.attn_align(*args, pmax, amax, *tail, causal=True)
    with pytest.raises(_lib.TT2Error, match="pmax"):
        ops.attn_align(*args, pmax.view(-1)[:-1], amax, *tail)
    with pytest.raises(_lib.TT2Error, match="amax"):
        ops.attn_align(*args, pmax, amax.float(), *tail)
    with pytest.raises(_lib.TT2Error, match="lse"):
        ops.attn_align(args[0], args[1], [P.lse.view(-1)[:-1]], pmax, amax, *tail)
    with pytest.raises(_lib.TT2Error, match="k\\[0\\]"):   # q f32, k bf16: a dtype mismatch
        ops.attn_align([P.q_d.float()], args[1], args[2], pmax, amax, *tail)
    with pytest.raises(_lib.TT2Error, match="at most 16"):
        ops.attn_align(args[0] * 17, args[1] * 17, args[2] * 17, pmax, amax, *tail)
    focus = torch.zeros(1, B, H, device="cuda")
    sel = torch.zeros(B, 2, dtype=torch.int32, device="cuda")
    sf = torch.zeros(B, device="cuda")
    dur = torch.zeros(B, Tk, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.TT2Error, match="durations"):
        ops.align_durations(pmax, amax, focus, sel, sf, dur.view(-1)[:-1], 1, B, H, Tq, Tk)
    with pytest.raises(_lib.TT2Error, match="sel"):
        ops.align_durations(pmax, amax, focus, sel.long(), sf, dur, 1, B, H, Tq, Tk)
    with pytest.raises(_lib.TT2Error, match="at most 16"):
        ops.align_durations(pmax, amax, focus, sel, sf, dur, 17, B, H, Tq, Tk)
    with pytest.raises(_lib.TT2Error, match="fixed head"):
        ops.align_durations(pmax, amax, focus, sel, sf, dur, 1, B, H, Tq, Tk, head=(1, 0))
