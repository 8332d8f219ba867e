"""tt2_attn_align, tt2_align_durations and tt2_guided_attn_loss held to exact and per-row bars (GPU).

The problems, numpy-float32 models and judges are tests/_align_refs.py's (validated on the CPU by
tests/test_align_refs.py, whose mutants prove that these bars reject the highest index of a tie, a
tie lost across the two lane halves, a dropped second durations chunk, a skipped (layer, head)
pair 17, 1 / tq for 1 / Ty_b and a count landing at t >= key_len):
  tt2_attn_align       exact: the selector problem with a supplied LSE, pmax = 2^-m and amax bit for
                       bit, ties across the 32-key halves, the lane halves and the 64-key tiles;
                       random: pmax per row, amax by the top-2-gap rule; (f32, 0) and (bf16, 0 .. 3)
                       at the six cross shapes, B = 4 with q_len above tq / in the middle / 0 /
                       negative, three layer slots whose K are column slices of one wide buffer
  tt2_align_durations  everything exact from hand-made pmax / amax, at the smallest shapes that
                       reach each second trip (17, 24 and 1024 pairs; 1030 rows; 2049 and 4100 keys)
  tt2_guided_attn_loss rows of small integers: term, coef and loss_out[0] bit-equal to the model
Every output is NaN-filled between NaN guards; every input the contract says is not read is NaN
(Q rows at and past q_len[b], K rows at and past key_len[b], the columns around the heads, pmax /
amax rows at and past q_len[b], the unguided heads' g rows).  pytest -s prints the worst ratios."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _align_refs as A  # noqa: E402
import _attn_refs as R  # noqa: E402
from _attn_refs import HEADS as H, D, F64  # noqa: E402
from tt2 import _lib, ops  # noqa: E402

B, L, HD = 4, 3, H * D
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
NAN = float("nan")
NAN_BITS = 0x7fc00000
GUARD, COL_BEFORE, COL_AFTER = 4, 8, 8
RUNS = [(F32, 0)] + [(BF16, v) for v in (0, 1, 2, 3)]
RUN_IDS = ["f32-auto", "bf16-auto", "bf16-v1", "bf16-v3w2", "bf16-v3w4"]
SHAPES = [(tq, tk, R.key_len_options(tk)[i % 4]) for i, (tq, tk) in enumerate(R.CROSS_TQ_TK)]
SHAPE_IDS = [f"{tq}x{tk}" for tq, tk, _ in SHAPES]


def b4(kl):
    return None if kl is None else list(kl) + list(kl)[::-1]


def guarded(n, dtype, fill=NAN):
    """A filled buffer and its [n] slice between guards."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, fill=None):
    x = buf.cpu()
    edge = torch.cat([x[:GUARD], x[-GUARD:]])
    return bool(torch.isnan(edge).all() if fill is None else (edge == fill).all())


def layer_of(x, l):
    """Layer slot l holds the problem with its heads rolled by l (dim 1 of [B, H, ...])."""
    return x.roll(l, 1)


class AlignLaunch:
    """L layer slots: Q of each in its own [B tq + 2, 8 + HD + 8] buffer, K of all as column slices of
    one wide [B tk + 2, 8 + L HD + 8] buffer; NaN around the heads' columns, past the last row, on
    the Q rows at and past q_len[b] and on the K rows at and past key_len[b]."""

    def __init__(self, p, lse, q_len, dtype):
        _, _, self.tq, self.tk = p.shape
        tq, tk = self.tq, self.tk
        self.dtype, self.scale = dtype, p.scale
        tx, ty = R.key_limits(B, tk, p.key_len), R.key_limits(B, tq, q_len)
        wide = torch.full((B * tk + 2, COL_BEFORE + L * HD + COL_AFTER), NAN, dtype=dtype)
        self.qs, self.lses = [], []
        for l in range(L):
            q = layer_of(p.q, l).transpose(1, 2).reshape(B, tq, HD).to(dtype)
            k = layer_of(p.k, l).transpose(1, 2).reshape(B, tk, HD).to(dtype)
            for b in range(B):
                q[b, int(ty[b]):] = NAN
                k[b, int(tx[b]):] = NAN
            qbuf = torch.full((B * tq + 2, COL_BEFORE + HD + COL_AFTER), NAN, dtype=dtype)
            qbuf[:B * tq, COL_BEFORE:COL_BEFORE + HD] = q.view(B * tq, HD)
            wide[:B * tk, COL_BEFORE + l * HD:COL_BEFORE + (l + 1) * HD] = k.view(B * tk, HD)
            self.qs.append(qbuf.cuda()[:B * tq, COL_BEFORE:COL_BEFORE + HD])
            self.lses.append(layer_of(lse, l).reshape(B * H, tq).to(F32).cuda())
        wide = wide.cuda()
        self.ks = [wide[:B * tk, COL_BEFORE + l * HD:COL_BEFORE + (l + 1) * HD] for l in range(L)]
        if tk == 0:                                              # a non-NULL pointer is still required
            self.ks = [wide[:1, COL_BEFORE:COL_BEFORE + HD]] * L
        self.q_ld, self.k_ld = COL_BEFORE + HD + COL_AFTER, wide.shape[1]
        self.key_len = None if p.key_len is None else torch.tensor(p.key_len, dtype=I32).cuda()
        self.q_len = None if q_len is None else torch.tensor(q_len, dtype=I32).cuda()

    def run(self, variant, lses=None):
        n = L * B * H * self.tq
        self.pbuf, pmax = guarded(n, F32)
        self.abuf, amax = guarded(n, I32, NAN_BITS)
        ops.attn_align(self.qs, self.ks, self.lses if lses is None else lses, pmax, amax, self.q_ld, self.k_ld, B, H,
                       self.tq, self.tk, key_len=self.key_len, q_len=self.q_len, scale=self.scale, variant=variant)
        torch.cuda.synchronize()
        assert guards_intact(self.pbuf) and guards_intact(self.abuf, NAN_BITS), "written outside pmax / amax"
        pm, am = pmax.cpu().view(L, B, H, self.tq), amax.cpu().view(L, B, H, self.tq)
        assert not torch.isnan(pm).any() and not (am == NAN_BITS).any(), "pmax / amax not fully written"
        return pm, am


# ------------------------------------------------------------------ tt2_attn_align, exact
@functools.lru_cache(maxsize=None)
def exact_problem(tq, tk, kl, dup=True):
    p, lse = A.align_exact_problem(B, H, tq, tk, None if kl is None else list(kl), dup)
    return p, lse, A.align_exact_expected(p, lse, A.align_q_len(tq))


@pytest.mark.parametrize("dtype,variant", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_align_exact(shape, dtype, variant):
    """pmax = 2^-m and amax bit for bit on every layer slot; rows >= q_len[b], +inf rows and
    utterances without a key give exactly +0 and -1."""
    tq, tk, kl = shape
    p, lse, (want_p, want_a) = exact_problem(tq, tk, None if kl is None else tuple(b4(kl)))
    pm, am = AlignLaunch(p, lse, A.align_q_len(tq), dtype).run(variant)
    for l in range(L):
        fails = A.judge_align_exact(pm[l], am[l], layer_of(want_p, l), layer_of(want_a, l))
        assert not fails, (l, fails)


@pytest.mark.parametrize("dtype,variant", RUNS, ids=RUN_IDS)
def test_align_no_keys(dtype, variant):
    """tk = 0: every row is (+0, -1)."""
    p = R.Problem(torch.zeros(B, H, 33, D, dtype=F64), torch.zeros(B, H, 0, D, dtype=F64), None, None, None, False, 0.125)
    pm, am = AlignLaunch(p, torch.zeros(B, H, 33, dtype=F64), A.align_q_len(33), dtype).run(variant)
    assert (pm.view(I32) == 0).all() and (am == -1).all()


@pytest.mark.parametrize("dtype,variant", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("shape", SHAPES[1:5], ids=SHAPE_IDS[1:5])
def test_align_exact_with_the_forwards_lse(shape, dtype, variant):
    """The forward's own LSE on the selector problem (no duplicated keys): pmax within 4 f32 ulp of
    1 or 1/2, amax as before.  Measured on an MI355X: 0 ulp on every run (355 ulp on the MFMA
    kernels before the contraction of s_max c - lse into one fma was switched off)."""
    tq, tk, kl = shape
    p, lse, _ = exact_problem(tq, tk, None if kl is None else tuple(b4(kl)), False)
    q_len = A.align_q_len(tq)
    run = AlignLaunch(p, lse, q_len, dtype)
    flat = lambda x, t: x.transpose(1, 2).reshape(B * t, HD).to(dtype).cuda()   # noqa: E731
    lses = []
    for l in range(L):
        out = torch.empty(B * tq, HD, dtype=dtype, device="cuda")
        lses.append(torch.empty(B * H, tq, dtype=F32, device="cuda"))
        k = flat(layer_of(p.k, l), tk)
        ops.attn_fwd(flat(layer_of(p.q, l), tq), k, k, out, lses[-1], HD, HD, HD, HD, B, H, tq, tk, run.key_len, False, p.scale)
    pm, am = run.run(variant, lses)
    valid = A.align_valid(B, H, tq, tk, p.key_len, q_len)
    s = A.masked_scores(p)
    ties = ((s == s.amax(-1, keepdim=True)) & torch.isfinite(s)).sum(-1)
    assert set(ties[valid].unique().tolist()) <= {1, 2}
    want_p = torch.where(valid, 1.0 / ties.clamp_min(1), torch.zeros(B, H, tq, dtype=F64))
    want_a = torch.where(valid, A.lowest_argmax(s), torch.full((B, H, tq), -1))
    worst = 0.0
    for l in range(L):
        assert torch.equal(am[l].long(), layer_of(want_a, l))
        d = R.ulp_distance(pm[l], layer_of(want_p, l), F32)
        assert (pm[l][~layer_of(valid, l)].view(I32) == 0).all()
        worst = max(worst, d.max().item())
    print(f"\nown lse {tq}x{tk}: pmax {worst:.2f} f32 ulp from 1 or 1/2")
    assert worst <= 4


# ------------------------------------------------------------------ tt2_attn_align, random
@functools.lru_cache(maxsize=None)
def random_problem(tq, tk, kl, dtype):
    p = R.random_problem(B, H, tq, tk, None if kl is None else list(kl), False, dtype)
    return p, A.align_random_reference(p, A.align_q_len(tq))


@pytest.mark.parametrize("dtype,variant", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_align_random(shape, dtype, variant):
    """The LSE is the float64 one rounded to float32, so only the kernel's dot product and exp2 are
    under test: pmax per row within max(4 x the float32 evaluations' error on that row, 2 f32 ulp
    -- judge_align_random says of what), amax by the top-2-gap rule.  Then the end-to-end
    invariant on the kernel's own output: sum_t durations = Ty_b iff Tx_b > 0.
    Measured on an MI355X: worst row at 0.28 of its bar; no row under the gap."""
    tq, tk, kl = shape
    p, ref = random_problem(tq, tk, None if kl is None else tuple(b4(kl)), dtype)
    q_len = A.align_q_len(tq)
    run = AlignLaunch(p, ref["lse"].to(F64), q_len, dtype)
    pm, am = run.run(variant)
    worst = {}
    for l in range(L):
        rl = {k: ([layer_of(e, l) for e in v] if k == "evals" else layer_of(v, l)) for k, v in ref.items()}
        fails, figs = A.judge_align_random(pm[l], am[l], rl)
        assert not fails, (l, fails, figs)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in figs.items()}
    print(f"\nrandom {tq}x{tk}: {R.show(worst)}")
    n = L * B * H * tq
    focus, sel, sel_focus, dur = torch.empty(L * B * H, device="cuda"), torch.empty(2 * B, dtype=I32, device="cuda"), \
        torch.empty(B, device="cuda"), torch.empty(B * tk, dtype=I32, device="cuda")
    ops.align_durations(run.pbuf[GUARD:GUARD + n], run.abuf[GUARD:GUARD + n], focus, sel, sel_focus, dur, L, B, H, tq, tk,
                        key_len=run.key_len, q_len=run.q_len)
    tx, ty = R.key_limits(B, tk, p.key_len), R.key_limits(B, tq, q_len)
    assert dur.view(B, tk).sum(-1).cpu().tolist() == [int(y) if x > 0 else 0 for x, y in zip(tx, ty)]


def test_align_refusals_leave_the_outputs_untouched():
    p, lse, _ = exact_problem(33, 64, None)
    run = AlignLaunch(p, lse, A.align_q_len(33), BF16)
    n = L * B * H * 33
    for kw in (dict(causal=True), dict(scale=0.0), dict(scale=-0.125), dict(q_ld=run.q_ld + 1), dict(k_ld=run.k_ld + 1)):
        pbuf, pmax = guarded(n, F32)
        abuf, amax = guarded(n, I32, NAN_BITS)
        args = dict(q_ld=run.q_ld, k_ld=run.k_ld, scale=0.125, causal=False)
        args.update(kw)
        with pytest.raises(_lib.TT2Error, match="tt2_attn_align"):
            ops.attn_align(run.qs, run.ks, run.lses, pmax, amax, args["q_ld"], args["k_ld"], B, H, 33, 64,
                           key_len=run.key_len, q_len=run.q_len, causal=args["causal"], scale=args["scale"], variant=0)
        torch.cuda.synchronize()
        assert torch.isnan(pbuf).all() and (abuf == NAN_BITS).all(), kw


# ------------------------------------------------------------------ tt2_align_durations
INT_FILL = -7777


@pytest.mark.parametrize("c", A.DUR_CASES, ids=lambda c: c["name"])
def test_durations_exact(c):
    """focus bit-equal to the numpy-float32 model; sel, sel_focus and durations from the model's
    focus; all four outputs fully written between intact guards; the NaN / huge-index rows at and
    past q_len[b] are not read."""
    Lc, Bc, Hc, tq, tk = (c[k] for k in ("L", "B", "H", "tq", "tk"))
    pmax, amax = A.durations_inputs(c)
    want = A.durations_model(c, pmax, amax)
    dev = lambda x, dt: None if x is None else torch.tensor(x, dtype=dt).cuda()   # noqa: E731
    fbuf, focus = guarded(Lc * Bc * Hc, F32)
    sbuf, sel = guarded(2 * Bc, I32, INT_FILL)
    sfbuf, sel_focus = guarded(Bc, F32)
    dbuf, dur = guarded(Bc * tk, I32, INT_FILL)
    outs = []
    for _ in range(2):
        ops.align_durations(pmax.to(F32).cuda().view(-1), amax.to(I32).cuda().view(-1), focus, sel, sel_focus, dur, Lc, Bc, Hc,
                            tq, tk, key_len=dev(c["key_len"], I32), q_len=dev(c["q_len"], I32), head=c["head"])
        torch.cuda.synchronize()
        outs.append([x.clone().cpu() for x in (fbuf, sbuf, sfbuf, dbuf)])
    assert all(torch.equal(x.view(I32), y.view(I32)) for x, y in zip(*outs)), "a second launch differs"
    assert guards_intact(fbuf) and guards_intact(sfbuf) and guards_intact(sbuf, INT_FILL) and guards_intact(dbuf, INT_FILL)
    assert not torch.isnan(focus).any() and not torch.isnan(sel_focus).any()
    assert not (sel == INT_FILL).any() and not (dur == INT_FILL).any(), "sel / durations not fully written"
    got = {"focus": focus.cpu().view(Lc, Bc, Hc).numpy(), "sel": sel.cpu().view(Bc, 2).numpy(),
           "sel_focus": sel_focus.cpu().numpy(), "durations": dur.cpu().view(Bc, tk).numpy()}
    fails = A.judge_durations(got, want)
    assert not fails, fails


def test_durations_refusals_leave_the_outputs_untouched():
    c = A.DUR_CASES[1]
    Lc, Bc, Hc, tq, tk = (c[k] for k in ("L", "B", "H", "tq", "tk"))
    pmax, amax = (x.cuda().view(-1) for x in (A.durations_inputs(c)[0].to(F32), A.durations_inputs(c)[1].to(I32)))
    for head in ((Lc, 0), (0, Hc), (-1, 0), (0, -1)):
        bufs = [guarded(Lc * Bc * Hc, F32), guarded(2 * Bc, I32, INT_FILL), guarded(Bc, F32), guarded(Bc * tk, I32, INT_FILL)]
        with pytest.raises(_lib.TT2Error, match="tt2_align_durations"):
            ops.align_durations(pmax, amax, *(b[1] for b in bufs), Lc, Bc, Hc, tq, tk, head=head)
        torch.cuda.synchronize()
        assert torch.isnan(bufs[0][0]).all() and torch.isnan(bufs[2][0]).all()
        assert (bufs[1][0] == INT_FILL).all() and (bufs[3][0] == INT_FILL).all()


# ------------------------------------------------------------------ tt2_guided_attn_loss
def loss_buffers(c, rows):
    """Per layer a NaN buffer holding [B H, tq] at `offset` floats from its 16-byte aligned start
    (+ guards); term, coef and loss_out as slices between NaN guards."""
    n = c["B"] * c["H"] * c["tq"]
    layers = []
    for l in range(c["L"]):
        buf = torch.full((n + 8,), NAN, dtype=F32)
        buf[4 + c["offset"]:4 + c["offset"] + n] = rows[l].reshape(-1).to(F32)
        buf = buf.cuda()
        assert buf.data_ptr() % 16 == 0
        layers.append(buf[4 + c["offset"]:4 + c["offset"] + n])
    return layers


@pytest.mark.parametrize("c", A.LOSS_CASES, ids=lambda c: c["name"])
def test_guided_loss_exact(c):
    """term, coef and loss_out[0] bit-equal to the numpy-float32 model; loss_out[1:] and the guards
    untouched; N = 0 leaves loss_out alone; the unguided heads' NaN rows are not read."""
    rows = A.loss_rows(c)
    term_w, coef_w, loss_w = A.loss_model(c, rows)
    layers = loss_buffers(c, rows)
    assert all((r.data_ptr() % 16 == 0) == (c["offset"] == 0) for r in layers)
    dev = lambda x: None if x is None else torch.tensor(x, dtype=I32).cuda()   # noqa: E731
    tbuf, term = guarded(1, F32)
    cbuf, coef = guarded(1, F32)
    lbuf, loss = guarded(4, F32)
    seen = []
    for _ in range(2):
        if c["loss0"] is not None:
            loss.copy_(torch.tensor([c["loss0"], 1.0, 1.0, 1.0]))
        ops.guided_attn_loss(layers, term, coef, c["B"], c["H"], c["tq"], c["tk"], key_len=dev(c["key_len"]),
                             q_len=dev(c["q_len"]), guide_heads=c["gh"], scale=c["scale"], grad_scale=c["grad_scale"],
                             loss_out=None if c["loss0"] is None else loss)
        torch.cuda.synchronize()
        seen.append((term.cpu().numpy().copy(), coef.cpu().numpy().copy(), loss.cpu().numpy().copy()))
    t, k, lo = seen[0]
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(*seen)), "a second launch differs"
    assert guards_intact(tbuf) and guards_intact(cbuf) and guards_intact(lbuf)
    assert t.view(np.int32)[0] == np.float32(term_w).view(np.int32), (t[0], term_w)
    assert k.view(np.int32)[0] == np.float32(coef_w).view(np.int32), (k[0], coef_w)
    if c["loss0"] is None:
        assert np.isnan(lo).all()
    else:
        assert lo.view(np.int32)[0] == np.float32(loss_w).view(np.int32) and lo[1:].tolist() == [1.0, 1.0, 1.0], (lo, loss_w)


def test_guided_loss_refusals_leave_the_outputs_untouched():
    c = A.LOSS_CASES[0]
    layers = loss_buffers(c, A.loss_rows(c))
    for kw in (dict(guide_heads=c["H"] + 1), dict(guide_heads=-1), dict(tq=-1), dict(tk=-1)):
        tbuf, term = guarded(1, F32)
        cbuf, coef = guarded(1, F32)
        lbuf, loss = guarded(4, F32)
        args = dict(guide_heads=c["gh"], tq=c["tq"], tk=c["tk"])
        args.update(kw)
        a = _lib.GuideLossArgs()
        for i, r in enumerate(layers):
            a.rows[i] = r.data_ptr()
        a.loss_out, a.term, a.coef = loss.data_ptr(), term.data_ptr(), coef.data_ptr()
        a.n_layers, a.batch, a.heads, a.guide_heads, a.tq, a.tk = c["L"], c["B"], c["H"], args["guide_heads"], args["tq"], args["tk"]
        a.scale, a.grad_scale = 10.0, 1.0
        rc = ops.lib().tt2_guided_attn_loss(ctypes.byref(a), ops.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.E_INVALID and b"tt2_guided_attn_loss" in ops.lib().tt2_last_error(), kw
        assert torch.isnan(tbuf).all() and torch.isnan(cbuf).all() and torch.isnan(lbuf).all(), kw
