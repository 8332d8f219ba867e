"""tests/_decode_refs.py against independent implementations (torch's scaled_dot_product_attention,
F.linear, _attn_refs.ref64), its exact-problem builders at every case of the GPU test, and the
proof that its judges bite: eleven deliberately wrong copies of the references, each of which the
exact problems that tests/test_gpu_decode_exact.py applies to the kernels must reject, while the
old whole-tensor bar of tests/test_gpu_decode_kernels.py accepts a key lost from, or leaked into,
one work group at 257 keys (CPU only)."""
import pytest
import torch
import torch.nn.functional as F

import _attn_refs as A
import _decode_refs as R
from _decode_refs import BF16, D, F16, F32, F64

H8 = 8


# ------------------------------------------------------------------ the references against torch
def _flat(p):
    B, H, T = p.shape
    return p.query().reshape(B, H * D), p.k.reshape(B, T, H * D), p.v.reshape(B, T, H * D)


def test_ref_attn_decode_is_sdpa():
    p = R.random_problem(4, [37, 1, 0], F32, T=40, wo=True)
    q, K, V = _flat(p)
    got = R.ref_attn_decode(q, K, V, p.nk, p.scale)
    for b, n in enumerate(p.nk):
        if n == 0:
            assert got[b].abs().max() == 0
            continue
        o = F.scaled_dot_product_attention(p.q[b][:, None, :], p.k[b, :n].transpose(0, 1), p.v[b, :n].transpose(0, 1),
                                           scale=p.scale)
        assert (got[b] - o.reshape(-1)).abs().max().item() < 1e-12
    ev = R.evaluate(p)
    assert (ev["o"].reshape(3, -1) - got).abs().max().item() < 1e-12
    assert (ev["slab"] - R.ref_slabs(got, p.wo)).abs().max().item() < 1e-12
    assert (R.ref_slabs(got, p.wo).sum(0) - got @ p.wo.t()).abs().max().item() < 1e-12
    # the training-side reference with Tq = 1
    pa = A.Problem(p.q[:, :, None, :], p.k.transpose(1, 2), p.v.transpose(1, 2), torch.zeros(3, 4, 1, D, dtype=F64),
                   p.nk, False, p.scale)
    assert (A.ref64(pa)["o"][:, :, 0] - ev["o"]).abs().max().item() < 1e-12
    stopped = R.ref_attn_decode(q, K, V, p.nk, p.scale, [False, True, False])
    assert torch.equal(stopped[0], got[0]) and stopped[1].abs().max() == 0


def test_ref_qproj_is_linear():
    p = R.random_problem(H8, [5, 9, 2], BF16, T=16, wq=True)
    q = R.ref_qproj(p.x, p.wq, p.bq)
    assert (q - F.linear(p.x, p.wq, p.bq)).abs().max().item() < 1e-12
    assert (p.query().reshape(3, -1) - q).abs().max().item() < 1e-12


def test_ref_kv_append():
    cache = torch.full((2, 4, 6), float("nan"))
    src = torch.arange(16.0).view(2, 8)
    out = R.ref_kv_append(cache, src, 2, 5)
    assert torch.equal(out[:, 2, :5], src[:, :5]) and int(torch.isnan(out).sum()) == 2 * 4 * 6 - 10
    for t in (4, 7):
        assert torch.isnan(R.ref_kv_append(cache, src, t, 5)).all()


def _script_heads(B, n_mels=80, seed=0):
    coarse, fine, bias, want = R.emit_script(B)
    g = torch.Generator().manual_seed(seed)
    steps = []
    for s in range(coarse.shape[0]):
        h = torch.randn(B, n_mels + 4, generator=g)
        h[:, n_mels] = (coarse[s] + fine[s]).to(F32)
        steps.append(h)
    return steps, bias, want


def test_ref_emit_follows_the_header():
    B, nm = 4, 80
    steps, bias, want = _script_heads(B)
    assert steps[0][0, nm].item() < R.EMIT_THR == steps[1][0, nm].item()
    assert steps[0][0, nm].item() == torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)).item()
    sl0 = torch.full((B,), R.INT32_MAX, dtype=torch.int32)
    states = R.emit_sequence(R.ref_emit, steps, R.EMIT_TMAX, nm, bias, sl0, R.EMIT_THR, 0xFFFFFFFE, BF16)
    last = states[-1]
    assert torch.equal(last["stop_len"], want) and last["t"] == R.EMIT_TMAX
    assert last["seed"] == (0xFFFFFFFE + R.EMIT_TMAX) & 0xFFFFFFFF == 2          # uint32 wrap
    assert not R.same_state(states[-1], states[-2])                               # the step at t_max changes nothing
    for t in range(R.EMIT_TMAX):
        for b in range(B):
            zero = want[b] <= t
            assert torch.equal(last["mel_seq"][b, t], torch.zeros(nm) if zero else steps[t][b, :nm])
            assert last["stop_seq"][b, t] == steps[t][b, nm] + bias[b, t]
    assert torch.equal(last["prev"], last["mel_seq"][:, -1].to(BF16))
    # without stop_len nothing is zeroed; without seed and bias
    free = R.emit_sequence(R.ref_emit, steps, R.EMIT_TMAX, nm, None, None, R.EMIT_THR, None)[-1]
    assert torch.equal(free["mel_seq"], torch.stack([s[:, :nm] for s in steps[:-1]], 1))
    assert free["seed"] is None and free["stop_len"] is None


# ------------------------------------------------------------------ exact-problem builders
def test_seam_keys():
    assert R.wave_ranges(65)[:2] == [(0, 16), (16, 32)] and R.wave_ranges(257)[6] == (240, 257)
    assert R.wave_ranges(513)[0] == (0, 72) and R.wave_ranges(513)[7] == (504, 513)
    s = R.seam_keys(513)
    assert {0, 512, 71, 72, 503, 504, 31, 32, 63, 64}.issubset(s) and len(set(s)) == len(s)
    assert R.seam_keys(0) == [] and R.seam_keys(1) == [0]
    for n in R.NK:
        assert all(0 <= k < n for k in R.seam_keys(n))


@pytest.mark.parametrize("case", R.cases(R.SELECTOR_ROT), ids=lambda c: c[0])
def test_selector_problem_is_exact(case):
    """The self-checks of the builder at every case of the GPU test, in every form it runs, and a
    float32 evaluation (in two summation orders) returns the float64 result bit for bit."""
    _, i, nk, form, dtype = case
    for H, wo, wq in ((H8, False, False), (H8, True, False), (4, True, False), (H8, True, True)):
        p = R.selector_problem(H, nk, rot=i, wo=wo, wq=wq)
        ref = R.assert_exact_selector(p, dtype)
        for ev in R.float32_evaluations(p, 2):
            assert torch.equal(ev["o"], ref["o"])
            assert ev["slab"] is None or torch.equal(ev["slab"], ref["slab"])
        rows = {tuple(r.tolist()) for b in range(3) for r in p.v[b, :max(nk[b], 1)].reshape(-1, D)}
        assert len(rows) == sum(max(n, 1) for n in nk) * H                  # V rows distinct per key, head, batch


def test_selector_visits_every_seam():
    """Over the batch slots, heads and rotations of the GPU test every seam of every count is the
    selected key at least once."""
    for i, n in enumerate(R.NK):
        seen = set()
        for rot in range(0, 48, 8):
            seen |= set(R.selector_problem(H8, [n] * 3, rot=rot).sel.reshape(-1).tolist())
        assert seen - {-1} == set(R.seam_keys(n)), n


def _slab_in_lane_order(o, wo):
    """The projection as the header's sum of 64 float32 products taken eight in a row and the
    eight partials pairwise (the shape of a lane-parallel sum): the 4-ulp bar of the uniform
    problem's slabs is for sums of that depth, not for 64 terms added one after the other, which
    reach 4.5 ulp on these inputs."""
    B, H, _ = o.shape
    N = wo.shape[0]
    a, w = o.view(B, H, 1, 8, 8), wo.view(N, H, 8, 8).permute(1, 0, 2, 3)[None]
    part = torch.zeros(B, H, N, 8, dtype=F32)
    for j in range(8):
        part = part + a[..., j] * w[..., j]
    for _ in range(3):
        part = part[..., 0::2] + part[..., 1::2]
    return part[..., 0].permute(1, 0, 2).to(F64)


def model(p, dtype, weights=None, perms=None, round_proj=None):
    """A float32 model of a correct kernel, or with `weights` / `round_proj` of a wrong one:
    R.evaluate in float32, o rounded to `dtype` at the store, the slabs from the unrounded o in
    lane order."""
    o32 = R.evaluate(p, F32, weights=weights, perms=perms)["o"].to(F32)
    out = {"o": o32.to(F64) if dtype == F32 else o32.to(dtype).to(F64), "slab": None}
    if p.wo is not None:
        out["slab"] = _slab_in_lane_order(o32 if round_proj is None else o32.to(round_proj).to(F32), p.wo.to(F32))
    return out


@pytest.mark.parametrize("case", R.cases(R.UNIFORM_ROT), ids=lambda c: c[0])
def test_uniform_problem_closed_form(case):
    _, i, nk, form, dtype = case
    for wo in (False, True):
        p = R.uniform_problem(H8, nk, wo=wo)
        R.assert_exact_uniform(p)
        ref = R.evaluate(p)
        assert (ref["o"] - R.uniform_expected(p)).abs().max().item() < 1e-14
        fails, figs = R.judge_uniform(model(p, dtype), p, dtype)
        print(f"\nuniform {case[0]} wo={wo}: {R.show(figs)}")
        assert not fails, fails


# ------------------------------------------------------------------ mutants of the attention
ONE = (1, 2)        # the (batch, head) whose work group the key mutants break: the others stay right


def drop_last_key_of_a_wave(p, dtype):          # the last non-empty wave stops one key short of its range
    w = R.counts_weights(p)
    live = [(a, e) for a, e in R.wave_ranges(p.nk[ONE[0]]) if a < e]
    if live:
        w[ONE[0], ONE[1], live[-1][1] - 1] = 0
    return model(p, dtype, weights=w)


def leak_one_key(p, dtype):                     # key nk[b] is admitted
    w = R.counts_weights(p)
    if p.nk[ONE[0]] < p.shape[2]:
        w[ONE[0], ONE[1], p.nk[ONE[0]]] = 1
    return model(p, dtype, weights=w)


def count_clamped_key_twice(p, dtype):          # the clamped duplicate of the last key is not masked
    w = R.counts_weights(p)
    n = p.nk[ONE[0]]
    if n > 0 and n % 8:
        w[ONE[0], ONE[1], n - 1] = 2
    return model(p, dtype, weights=w)


def merge_without_factor(p, dtype):             # the waves' partials are summed without exp2(m_i - M)
    B, H, T = p.shape
    q = p.query(F32)
    c = torch.tensor(p.scale, dtype=F32) * torch.tensor(R.LOG2E, dtype=F32)
    o = torch.zeros(B, H, D, dtype=F32)
    for b, n in enumerate(p.nk):
        L, O = torch.zeros(H, 1), torch.zeros(H, D)
        for a, e in R.wave_ranges(n):
            if a < e:
                s = torch.einsum("hd,thd->ht", q[b], p.k[b, a:e].to(F32)) * c
                pe = torch.exp2(s - s.amax(-1, keepdim=True))
                L, O = L + pe.sum(-1, keepdim=True), O + torch.einsum("ht,thd->hd", pe, p.v[b, a:e].to(F32))
        if n > 0:
            o[b] = O / L
    out = {"o": o.to(F64) if dtype is None else o.to(dtype).to(F64), "slab": None}
    if p.wo is not None:
        out["slab"] = _slab_in_lane_order(o, p.wo.to(F32))
    return out


def heads_swapped(p, dtype):                    # heads 0 and 1 of batch element 1 trade places
    out = model(p, dtype)
    out["o"][1, [0, 1]] = out["o"][1, [1, 0]]
    if out["slab"] is not None:
        out["slab"][[0, 1], 1] = out["slab"][[1, 0], 1]
    return out


def key_len_of_the_neighbour(p, dtype):         # key_len[b] is applied to b + 1
    w = R.counts_weights(p, p.nk[-1:] + p.nk[:-1])
    return model(p, dtype, weights=w)


def round_o_before_projection(p, dtype):        # the projection reads the rounded head output
    return model(p, dtype, round_proj=BF16)


ATTN_MUTANTS = [drop_last_key_of_a_wave, leak_one_key, count_clamped_key_twice, merge_without_factor, heads_swapped,
                key_len_of_the_neighbour, round_o_before_projection]
MUTANT_NK = ([257, 257, 257], [513, 65, 9])
_cache = {}


def _problems():
    """[(kind, problem, float64 reference, twin, float32 evaluations)], bf16 with the fused output
    projection, built once."""
    if not _cache:
        rows = []
        for nk in MUTANT_NK:
            ps = R.selector_problem(H8, nk, wo=True, rot=3)
            rows.append(("selector", ps, R.assert_exact_selector(ps, BF16), None, None))
            pu = R.uniform_problem(H8, nk, wo=True)
            rows.append(("uniform", pu, None, None, None))
            pr = R.random_problem(H8, nk, BF16, wo=True)
            rows.append(("random", pr, R.evaluate(pr), R.twin(pr, BF16), R.float32_evaluations(pr)))
        _cache["rows"] = rows
    return _cache["rows"]


def _judge(kind, out, p, ref, tw, y32):
    if kind == "selector":
        return R.judge_selector(out, ref, BF16)
    if kind == "uniform":
        return R.judge_uniform(out, p, BF16)
    return R.judge_random(out, ref, tw, y32, BF16)


def test_a_float32_model_passes_every_judge():
    """The plain float32 evaluation rounded at the store, in a permuted summation order: what a
    correct kernel computes up to the order of its sums."""
    g = torch.Generator().manual_seed(9)
    for kind, p, ref, tw, y32 in _problems():
        T = p.shape[2]
        perms = (torch.randperm(D, generator=g), torch.randperm(T, generator=g), torch.randperm(R.DM, generator=g))
        fails, figs = _judge(kind, model(p, BF16, perms=perms), p, ref, tw, y32)
        assert not fails, (kind, p.nk, fails)


@pytest.mark.parametrize("mutant", ATTN_MUTANTS, ids=lambda m: m.__name__)
def test_attention_mutant_is_rejected(mutant):
    """Each wrong copy misses a bar of at least one EXACT problem (selector or uniform).  Printed
    (pytest -s): the problems that reject it and whether the old whole-tensor bar (rel < 1e-2 on
    random inputs) accepts it at nk = 257.

    Measured (B = 3, H = 8, bf16, fused Wo; nk = 257 x 3 and [513, 65, 9]; the three key mutants
    break the work group of (batch 1, head 2) alone):
      drop_last_key_of_a_wave    uniform, random, both shapes                 old bar accepts
      leak_one_key               selector, uniform, random, both shapes      old bar accepts
      count_clamped_key_twice    uniform, random, both shapes                 old bar accepts
      merge_without_factor       selector, random, both shapes                old bar rejects
      heads_swapped              selector, uniform, random, both shapes      old bar rejects
      key_len_of_the_neighbour   all three at [513, 65, 9] (257 x 3: no change)
      round_o_before_projection  uniform, random, both shapes                 old bar accepts
    The selector problem sees a dropped key where it is the selected one (the GPU test walks the
    selection over every seam, test_selector_visits_every_seam; here it is one fixed rotation).
    round_o_before_projection changes nothing where o is a bf16 value (selector); the uniform
    problem's slabs must be the sums of the unrounded means, bit for bit at a power-of-two count."""
    rejected, exact, old_accepts = [], False, True
    for kind, p, ref, tw, y32 in _problems():
        out = mutant(p, BF16)
        fails, _ = _judge(kind, out, p, ref, tw, y32)
        if fails:
            rejected.append(f"{kind}-{'x'.join(str(n) for n in p.nk)}")
            exact |= kind != "random"
        if kind == "random" and p.nk == MUTANT_NK[0]:
            old_accepts = R.old_global_bar(out, ref)
    print(f"\n{mutant.__name__:28s} rejected by: {', '.join(rejected) or 'nothing':90s} "
          f"old global bar at 257: {'accepts' if old_accepts else 'rejects'}")
    assert exact, rejected


def test_round_o_mutant_needs_a_power_of_two_count():
    """The uniform problem sees the rounded projection input through its bit-equal slabs."""
    p = R.uniform_problem(H8, [256, 64, 8], wo=True)
    assert not R.judge_uniform(model(p, BF16), p, BF16)[0]
    assert R.judge_uniform(round_o_before_projection(p, BF16), p, BF16)[0]


@pytest.mark.parametrize("mutant", [drop_last_key_of_a_wave, leak_one_key], ids=lambda m: m.__name__)
def test_old_bar_accepts_a_lost_or_leaked_key_at_257(mutant):
    """The gap this file closes: one key of 257 dropped from, or leaked into, one (batch, head) of the
    24 moves the random output by 0.5 % of its norm, under rel < 1e-2, while the per-vector bar
    rejects it.  (The same key lost in EVERY (batch, head) moves it by 6 %, which the old bar does
    see: with random V the output is a mean of 257 rows, of norm 1 / 16 of a row's.)"""
    kind, p, ref, tw, y32 = [r for r in _problems() if r[0] == "random" and r[1].nk == MUTANT_NK[0]][0]
    out = mutant(p, BF16)
    assert R.old_global_bar(out, ref)
    assert R.judge_random(out, ref, tw, y32, BF16)[0]


# ------------------------------------------------------------------ mutants of the emit
class StrictlyGreater(R.EmitRef):               # > for >=
    def stops(self, logit, thr):
        return logit > thr


class LaterStopOverwrites(R.EmitRef):           # stop_len follows the last stop, not the first
    def may_set(self, stop_len, t):
        return torch.ones_like(stop_len, dtype=torch.bool)


class FramesNotZeroed(R.EmitRef):               # frames after the stop keep their values
    def frames(self, mel, stop_len, t):
        return mel


class RunsPastTmax(R.EmitRef):                  # t (and the seed) advance at t = t_max
    def live(self, t, t_max):
        return True


@pytest.mark.parametrize("mutant", [StrictlyGreater, LaterStopOverwrites, FramesNotZeroed, RunsPastTmax],
                         ids=lambda m: m.__name__)
def test_emit_mutant_is_rejected(mutant):
    B, nm = 4, 80
    steps, bias, want = _script_heads(B)
    sl0 = torch.full((B,), R.INT32_MAX, dtype=torch.int32)
    good = R.emit_sequence(R.ref_emit, steps, R.EMIT_TMAX, nm, bias, sl0, R.EMIT_THR, 7, F16)
    bad = R.emit_sequence(mutant(), steps, R.EMIT_TMAX, nm, bias, sl0, R.EMIT_THR, 7, F16)
    diffs = [R.same_state(a, b) for a, b in zip(good, bad)]
    print(f"\n{mutant.__name__}: differs in {[d for d in diffs]}")
    assert any(diffs)
