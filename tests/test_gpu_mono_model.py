"""TransformerTTS.monotonic_durations() (GPU), on test_gpu_align_model.py's configurations: the
B = 2, 17 / 23 batch with lengths 11 / 15 and the B = 2, Tx = 70, Ty = 150 batch that spans several
key tiles, with the query projection of every decoder cross-attention multiplied by BOOST so the
attention is peaked.

f32 against the oracle: with eta the largest log-domain difference between the oracle's attention
weights and alignments() over the visible entries of the utterance's chosen head (measured here,
printed), either path's log-likelihood moves by at most Ty * eta between the two sets of weights,
and the search's own f32 rounding is covered by the 1e-5 per row: the returned path's
log-likelihood under the oracle's weights is within 2 Ty (eta + 1e-5) of the float64 optimum on
those weights.

bf16: logp against log(alignments()) gathered along the returned path (same q, k and LSE; only the
exp2 / log round trip differs), bar max(1e-5, 2 x the greatest log-domain distance between
alignment_stats().pmax and alignments().amax(-1) over the chosen head's valid rows of the same
forward), printed before it is asserted.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _mas_refs import check_path, durations_of, mas_path, path_score  # noqa: E402
from tt2 import ops  # noqa: E402
from tt2.config import TTSConfig  # noqa: E402
from tt2.model import MonotonicAlignment, TransformerTTS  # noqa: E402
from tt2_oracle import OracleConfig, TransformerTTSOracle, init_deterministic  # noqa: E402

BOOST = 32.0


def make_batch(B=2, Tx=17, Ty=23, text_len=(17, 11), mel_len=(23, 15), seed=0):
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(1, 80, (B, Tx), generator=g)
    tl, ml = torch.tensor(text_len), torch.tensor(mel_len)
    mel = torch.randn(B, Ty, 80, generator=g)
    for b in range(B):
        text[b, tl[b]:] = 0
        mel[b, ml[b]:] = 0
    return text, tl, mel, ml


BATCHES = {"small": dict(), "tiles": dict(Tx=70, Ty=150, text_len=(70, 41), mel_len=(150, 97), seed=1)}


@pytest.fixture(scope="module")
def oracle():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    o = init_deterministic(TransformerTTSOracle(OracleConfig()), 5)
    sd = o.state_dict()
    for k in sd:
        if ".cross_attn.in_proj_" in k and k.startswith("decoder.layers."):
            sd[k][:512] *= BOOST
    o.load_state_dict(sd)
    return o.eval()


def gpu_model(oracle, dtype):
    m = TransformerTTS(TTSConfig(), dtype=dtype)
    m.load_state_dict(oracle.state_dict())
    return m


@pytest.fixture(scope="module")
def m32(oracle):
    return gpu_model(oracle, torch.float32)


@pytest.fixture(scope="module")
def m16(oracle):
    m = gpu_model(oracle, torch.bfloat16)
    m.configure_optimizer(lr=1e-4, warmup=10.0)
    return m


def check_properties(r, tl, ml, Tx):
    """A valid path per utterance, its histogram as durations, every phoneme covered."""
    assert isinstance(r, MonotonicAlignment)
    path, dur = r.path.cpu().numpy().astype(np.int64), r.durations.cpu().numpy().astype(np.int64)
    assert r.path.dtype == torch.int32 and r.durations.dtype == torch.int32 and r.logp.dtype == torch.float32
    for b in range(len(tl)):
        ty, tx = int(ml[b]), int(tl[b])
        assert check_path(path[b, :ty], ty, tx) is None, (b, check_path(path[b, :ty], ty, tx))
        assert (path[b, ty:] == -1).all()
        assert np.array_equal(dur[b], durations_of(path[b, :ty], Tx))
        assert dur[b].sum() == ty and (dur[b, tx:] == 0).all()
        if ty >= tx:
            assert (dur[b, :tx] >= 1).all()
    assert torch.isfinite(r.logp).all() and (r.logp <= 1e-6).all()   # a mean of log-probabilities (f32 rounding)
    return path


def direct_call(m, layers=None):
    """ops.align_monotonic on the last forward's arena buffers, head choice from align_stats."""
    e, A, c = m.engine, m._last, m.cfg
    ls = e.align_layers(layers)
    st = e.align_stats(A, ls)
    d, H = c.d_model, c.n_heads
    path = torch.full((A.B, A.Ty), 77, dtype=torch.int32, device=e.dev)
    dur = torch.full((A.B, A.Tx), 77, dtype=torch.int32, device=e.dev)
    logp = torch.full((A.B,), 7.0, dtype=torch.float32, device=e.dev)
    ops.align_monotonic([A[f"dcq{l}"] for l in ls], [A["mkv"][:, 2 * d * l:] for l in ls],
                        [A[f"dclse{l}"] for l in ls], path, dur, logp, d, c.n_dec * 2 * d, A.B, H, A.Ty, A.Tx,
                        key_len=A["text_len"], q_len=A["mel_len"], sel=st["sel"], scale=1.0 / math.sqrt(c.head_dim))
    return path, dur, logp


@pytest.mark.parametrize("name", list(BATCHES))
def test_f32_against_the_oracle(oracle, m32, name):
    text, tl, mel, ml = make_batch(**BATCHES[name])
    with torch.no_grad():
        attn = oracle(text, tl, mel, ml, return_attn=True)[3]["dec_cross"]
    m32.train()
    d = m32.durations(text, tl.int(), mel, ml.int())
    r = m32.monotonic_durations(text, tl.int(), mel, ml.int())
    assert m32.training
    path = check_properties(r, tl, ml, text.shape[1])
    # the same head and focus as durations(), and the kernel's own outputs
    assert torch.equal(r.head, d.head) and torch.equal(r.focus, d.focus)
    for got, want in zip((r.path, r.durations, r.logp), direct_call(m32)):
        assert torch.equal(got, want)
    # the default path is what it was
    for a, b in zip(d, m32.durations(text, tl.int(), mel, ml.int())):
        assert torch.equal(a, b)
    head = r.head.cpu().tolist()
    for b in range(2):
        l, h = head[b]
        ty, tx = int(ml[b]), int(tl[b])
        p_or = attn[l][b, h, :ty, :tx].detach().double().cpu()
        p_al = m32.alignments(l)[b, h, :ty, :tx].double().cpu()
        assert (p_or > 0).all() and (p_al > 0).all(), "a visible weight underflowed: the log comparison is void"
        lp = p_or.log().numpy()
        eta = float((p_or.log() - p_al.log()).abs().max())
        best = mas_path(lp, ty, tx)
        gap = path_score(lp, best) - path_score(lp, path[b, :ty])
        bound = 2 * ty * (eta + 1e-5)
        print(f"f32 {name} b {b} head ({l}, {h}): eta {eta:.3e}, min weight {float(p_or.min()):.3e}, "
              f"L(pi*) - L(pi_gpu) = {gap:.3e}, bound {bound:.3e}, {int((best != path[b, :ty]).sum())} frames differ, "
              f"argmax-histogram zeros {int((d.durations[b, :tx] == 0).sum())}")
        assert -1e-9 <= gap <= bound, (gap, bound)


@pytest.mark.parametrize("name", list(BATCHES))
def test_bf16_logp_and_fixed_heads(m16, name):
    text, tl, mel, ml = make_batch(**BATCHES[name])
    m16.eval()
    r = m16.monotonic_durations(text, tl.int(), mel, ml.int())
    assert not m16.training
    path = check_properties(r, tl, ml, text.shape[1])
    for got, want in zip((r.path, r.durations, r.logp), direct_call(m16)):
        assert torch.equal(got, want)
    st = m16.alignment_stats()
    head = r.head.cpu().tolist()
    for b in range(2):
        l, h = head[b]
        ty, tx = int(ml[b]), int(tl[b])
        al = m16.alignments(l)[b, h, :ty].double().cpu()
        floor = float((st.pmax[l, b, h, :ty].double().cpu().log() - al.amax(-1).log()).abs().max())
        want = float(al.gather(1, torch.from_numpy(path[b, :ty]).view(-1, 1)).log().mean())
        err, bar = abs(float(r.logp[b]) - want), max(1e-5, 2 * floor)
        print(f"bf16 {name} b {b} head ({l}, {h}): logp {want:.5f}, err {err:.3e}, pmax floor {floor:.3e}, bar {bar:.3e}")
        assert err <= bar, (err, bar)
    # a fixed head, and a search restricted to one layer
    r2 = m16.monotonic_durations(text, tl.int(), mel, ml.int(), head=(3, 6))
    assert r2.head.cpu().tolist() == [[3, 6], [3, 6]]
    check_properties(r2, tl, ml, text.shape[1])
    r5 = m16.monotonic_durations(text, tl.int(), mel, ml.int(), layers=[5])
    d5 = m16.durations(text, tl.int(), mel, ml.int(), layers=[5])
    assert (r5.head[:, 0] == 5).all() and torch.equal(r5.head, d5.head) and torch.equal(r5.focus, d5.focus)
    check_properties(r5, tl, ml, text.shape[1])
    for got, want in zip((r5.path, r5.durations, r5.logp), direct_call(m16, layers=[5])):
        assert torch.equal(got, want)
    with pytest.raises(ValueError):
        m16.monotonic_durations(text, tl.int(), mel, ml.int(), head=(2, 1), layers=[5])
    m16.train()


def test_after_train_step_and_captured_replay(m16):
    text, tl, mel, ml = [x.cuda() for x in make_batch(**BATCHES["tiles"])]
    tl, ml = tl.int(), ml.int()
    m16.train()
    for _ in range(2):
        m16.train_step(text, tl, mel, ml)

    def check(what):
        # on the step's own saved buffers (dropout on), then through a forward of its own
        e = m16.engine
        out = e.align_monotonic(m16._last, e.align_layers(None))
        r = MonotonicAlignment(out["durations"], out["path"], out["sel"], out["sel_focus"], out["logp"])
        check_properties(r, tl.cpu(), ml.cpu(), text.shape[1])
        check_properties(m16.monotonic_durations(text, tl, mel, ml), tl.cpu(), ml.cpu(), text.shape[1])
        assert m16.training, what

    check("after train_step")
    run = m16.capture_train_step(2, 70, 150)
    loss = run(text, tl, mel, ml)
    check("after a captured replay")
    before = loss.clone()
    loss = run(text, tl, mel, ml)   # the captured step still replays
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and not torch.equal(loss, before)
    check("after the next replay")


def test_leaves_the_training_state_alone(oracle):
    text, tl, mel, ml = make_batch(**BATCHES["small"])
    tl, ml = tl.int(), ml.int()
    pair = []
    for _ in range(2):
        m = gpu_model(oracle, torch.bfloat16).train()
        m.configure_optimizer(lr=1e-3, warmup=10.0)
        m.set_seed(9)
        m.train_step(text, tl, mel, ml)
        pair.append(m)
    m, twin = pair
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    seed0 = m.engine.seed.clone()
    mom0 = (m.engine.exp_avg.clone(), m.engine.exp_avg_sq.clone(), m.engine.step_t.clone())
    r = m.monotonic_durations(text, tl, mel, ml)
    assert m.training and m.engine.training
    check_properties(r, tl, ml, text.shape[1])
    sd1 = m.state_dict()
    assert list(sd0) == list(sd1)
    for k in sd0:   # parameters, BatchNorm running statistics, num_batches_tracked
        assert torch.equal(sd0[k], sd1[k]), k
    assert torch.equal(seed0, m.engine.seed)
    for a, b in zip(mom0, (m.engine.exp_avg, m.engine.exp_avg_sq, m.engine.step_t)):
        assert torch.equal(a, b)
    la = m.train_step(text, tl, mel, ml).clone()
    lb = twin.train_step(text, tl, mel, ml).clone()
    assert torch.equal(la, lb), (la, lb)


def test_transient_keeps_no_arena_per_shape(m32):
    e = m32.engine
    text, tl, mel, ml = make_batch(**BATCHES["small"])
    m32.monotonic_durations(text, tl.int(), mel, ml.int())   # a shape the model holds
    held = set(e.arenas)
    assert (2, 17, 23) in held
    for j in range(2):
        tx, ty = 19 + 3 * j, 31 + 5 * j
        bt = make_batch(Tx=tx, Ty=ty, text_len=(tx, tx - 4), mel_len=(ty, ty - 9), seed=j)
        r = m32.monotonic_durations(bt[0], bt[1].int(), bt[2], bt[3].int(), transient=True)
        assert set(e.arenas) == held
        assert r.durations.sum(1).cpu().tolist() == [ty, ty - 9]
    plain = m32.monotonic_durations(bt[0], bt[1].int(), bt[2], bt[3].int())
    assert set(e.arenas) == held | {(2, 22, 36)}
    for a, b in zip(r, plain):
        assert torch.equal(a, b)
    again = m32.monotonic_durations(text, tl.int(), mel, ml.int(), transient=True)   # an existing arena stays
    assert (2, 17, 23) in e.arenas and int(again.durations.sum()) == int(ml.sum())
