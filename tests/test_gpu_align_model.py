"""TransformerTTS.alignment_stats() / durations() (GPU).

Batches: test_gpu_model.py's make_batch shape (B = 2, 17 / 23 with lengths 11 / 15) and one
B = 2, Tx = 70, Ty = 150 batch that spans several key tiles.

A randomly initialised cross-attention is nearly uniform, so the state dict that both the oracle
and the model load has the first 512 rows (the query projection) of every
decoder.layers.*.cross_attn.in_proj_weight / in_proj_bias multiplied by 32.

Rule (f32 against the oracle's return_attn weights; bf16 against model.alignments(l) of the same
forward, where q, k and the LSE are the same and only the summation order differs): argmax
equality on every valid row whose reference top-2 weights differ by >= 1e-3 relative; the other
rows ("exempt") are at most 5 % of the valid rows; focus within 1e-3; durations of a head within
2 x (that head's exempt rows) of the reference-derived ones in L1 (a row that flips moves one
count between two phonemes)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tt2.config import TTSConfig  # noqa: E402
from tt2.model import TransformerTTS  # noqa: E402
from tt2_oracle import OracleConfig, TransformerTTSOracle, init_deterministic  # noqa: E402

BOOST = 32.0
REL_GAP = 1e-3


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


def ref_stats(probs, tl, ml):
    """probs: per layer [B, H, Ty, Tx] (CPU).  argmax, relative top-2 gap, validity, focus."""
    p = torch.stack([x.detach().double().cpu() for x in probs])   # [L, B, H, Ty, Tx]
    L, B, H, Ty, Tx = p.shape
    top = p.topk(2, dim=-1)
    gap = (top.values[..., 0] - top.values[..., 1]) / top.values[..., 0].clamp_min(1e-300)
    valid = (torch.arange(Ty)[None, :] < ml[:, None]).view(1, B, 1, Ty).expand(L, B, H, Ty)
    focus = (top.values[..., 0] * valid).sum(-1) / ml.view(1, B, 1).clamp(min=1)
    return top.indices[..., 0], gap, valid, focus


def durations_of(arg, valid_n, Tx):
    return torch.bincount(arg[:valid_n], minlength=Tx)


def check_stats(st, ref, tl, ml, what):
    arg_ref, gap, valid, focus_ref = ref
    amax, pmax, focus = st.argmax.cpu().long(), st.pmax.cpu(), st.focus.cpu().double()
    assert (amax[~valid] == -1).all() and (pmax[~valid] == 0).all()
    clear = valid & (gap >= REL_GAP)
    exempt = valid & ~clear
    print(f"{what}: focus max {focus_ref.max().item():.3f}, exempt rows {int(exempt.sum())} of {int(valid.sum())}, "
          f"focus err {(focus - focus_ref).abs().max().item():.2e}")
    assert (amax[clear] == arg_ref[clear]).all(), int((amax[clear] != arg_ref[clear]).sum())
    assert int(exempt.sum()) <= 0.05 * int(valid.sum())
    assert (focus - focus_ref).abs().max().item() <= 1e-3
    return exempt


def check_durations(d, ref, tl, ml, exempt, Tx, layers=None):
    """d: Durations.  Each utterance's chosen head is (one of) the reference's best within the
    focus tolerance on both sides, and its durations are the reference-derived ones of that head
    up to 2 per exempt row."""
    arg_ref, _, _, focus_ref = ref
    dur, head, fc = d.durations.cpu().long(), d.head.cpu().long(), d.focus.cpu().double()
    B = dur.shape[0]
    for b in range(B):
        l, h = int(head[b, 0]), int(head[b, 1])
        pool = focus_ref[:, b] if layers is None else focus_ref[list(layers), b]
        assert focus_ref[l, b, h] >= pool.max() - 2e-3
        assert abs(fc[b] - focus_ref[l, b, h]) <= 1e-3
        want = durations_of(arg_ref[l, b, h], int(ml[b]), Tx)
        assert int((dur[b] - want).abs().sum()) <= 2 * int(exempt[l, b, h].sum()), (b, dur[b], want)
        assert int(dur[b].sum()) == int(ml[b]) and (dur[b, int(tl[b]):] == 0).all()


@pytest.mark.parametrize("name", list(BATCHES))
def test_f32_against_the_oracle(oracle, m32, name):
    text, tl, mel, ml = make_batch(**BATCHES[name])
    with torch.no_grad():
        attn = oracle(text, tl, mel, ml, return_attn=True)[3]["dec_cross"]
    ref = ref_stats(attn, tl, ml)
    m32.eval()
    with torch.no_grad():
        m32(text, tl.int(), mel, ml.int())
    st = m32.alignment_stats()
    assert st.layers == tuple(range(6)) and st.pmax.shape == (6, 2, 8, mel.shape[1])
    exempt = check_stats(st, ref, tl, ml, f"f32 {name}")
    assert ref[3].max() > 0.5   # the boosted attention is peaked: the argmax means something
    m32.train()
    d = m32.durations(text, tl.int(), mel, ml.int())
    assert m32.training
    check_durations(d, ref, tl, ml, exempt, text.shape[1])


@pytest.mark.parametrize("name", list(BATCHES))
def test_bf16_against_alignments(m16, name):
    text, tl, mel, ml = make_batch(**BATCHES[name])
    m16.eval()
    with torch.no_grad():
        m16(text, tl.int(), mel, ml.int())
    ref = ref_stats([m16.alignments(l) for l in range(6)], tl, ml)
    exempt = check_stats(m16.alignment_stats(), ref, tl, ml, f"bf16 {name}")
    d = m16.durations(text, tl.int(), mel, ml.int())   # the same forward again (eval, no dropout)
    assert not m16.training
    check_durations(d, ref, tl, ml, exempt, text.shape[1])
    # a fixed head, and a search restricted to one layer
    d2 = m16.durations(text, tl.int(), mel, ml.int(), head=(3, 6))
    assert d2.head.cpu().tolist() == [[3, 6], [3, 6]]
    check_stats(m16.alignment_stats(layers=[3]), tuple(x[3:4] for x in ref), tl, ml, "layer 3")
    for b in range(2):
        want = durations_of(ref[0][3, b, 6], int(ml[b]), text.shape[1])
        assert int((d2.durations[b].cpu().long() - want).abs().sum()) <= 2 * int(exempt[3, b, 6].sum())
    d5 = m16.durations(text, tl.int(), mel, ml.int(), layers=[5])
    assert (d5.head[:, 0] == 5).all()
    check_durations(d5, ref, tl, ml, exempt, text.shape[1], layers=[5])
    with pytest.raises(ValueError):
        m16.durations(text, tl.int(), mel, ml.int(), head=(2, 1), layers=[5])
    m16.train()


def test_stats_after_train_step_and_captured_replay(m16):
    text, tl, mel, ml = [x.cuda() for x in make_batch(**BATCHES["tiles"])]
    tl, ml = tl.int(), ml.int()
    m16.train()
    for _ in range(2):
        m16.train_step(text, tl, mel, ml)

    def check(what):
        ref = ref_stats([m16.alignments(l) for l in range(6)], tl.cpu(), ml.cpu())
        check_stats(m16.alignment_stats(), ref, tl.cpu(), ml.cpu(), what)

    check("after train_step")
    run = m16.capture_train_step(2, 70, 150)
    loss = run(text, tl, mel, ml)
    check("after a captured replay")
    before = loss.clone()
    loss = run(text, tl, mel, ml)   # the captured step still replays
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and not torch.equal(loss, before)
    check("after the next replay")


@pytest.mark.parametrize("guided", [False, True])
def test_durations_leaves_the_training_state_alone(oracle, guided):
    text, tl, mel, ml = make_batch(**BATCHES["small"])
    tl, ml = tl.int(), ml.int()
    pair = []
    for _ in range(2):
        m = gpu_model(oracle, torch.bfloat16).train()
        m.configure_optimizer(lr=1e-3, warmup=10.0)
        m.set_seed(9)
        if guided:
            m.guided_attention()
        m.train_step(text, tl, mel, ml)
        pair.append(m)
    m, twin = pair
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    seed0 = m.engine.seed.clone()
    mom0 = (m.engine.exp_avg.clone(), m.engine.exp_avg_sq.clone(), m.engine.step_t.clone())
    d = m.durations(text, tl, mel, ml)
    assert m.training and m.engine.training
    assert int(d.durations.sum()) == int(ml.sum())
    sd1 = m.state_dict()
    assert list(sd0) == list(sd1)
    for k in sd0:   # parameters, BatchNorm running statistics, num_batches_tracked
        assert torch.equal(sd0[k], sd1[k]), k
    assert torch.equal(seed0, m.engine.seed)
    for a, b in zip(mom0, (m.engine.exp_avg, m.engine.exp_avg_sq, m.engine.step_t)):
        assert torch.equal(a, b)
    # with guidance on the durations still come from the attention the guided kernels saved
    ref = ref_stats([m.alignments(l) for l in range(6)], tl.long(), ml.long())
    exempt = check_stats(m.alignment_stats(), ref, tl.long(), ml.long(), f"guided={guided}")
    check_durations(d, ref, tl.long(), ml.long(), exempt, text.shape[1])
    la = m.train_step(text, tl, mel, ml).clone()
    lb = twin.train_step(text, tl, mel, ml).clone()
    assert torch.equal(la, lb), (la, lb)


def test_transient_durations_keep_no_arena_per_shape(m32):
    """A corpus of ragged batches runs a new (B, Tx, Ty) per batch: with transient=True the engine
    keeps none of their arenas, the shapes it already ran keep theirs, and the results are those
    of a plain call."""
    e = m32.engine
    text, tl, mel, ml = make_batch(**BATCHES["small"])
    m32.durations(text, tl.int(), mel, ml.int())   # a shape the model holds (as its training shape would be)
    held = set(e.arenas)
    assert (2, 17, 23) in held
    for j in range(4):
        tx, ty = 19 + 3 * j, 31 + 5 * j
        bt = make_batch(Tx=tx, Ty=ty, text_len=(tx, tx - 4), mel_len=(ty, ty - 9), seed=j)
        d = m32.durations(bt[0], bt[1].int(), bt[2], bt[3].int(), transient=True)
        assert set(e.arenas) == held
        assert d.durations.sum(1).cpu().tolist() == [ty, ty - 9]
        assert m32.alignment_stats().pmax.shape[-1] == ty   # the last forward is still readable
    plain = m32.durations(bt[0], bt[1].int(), bt[2], bt[3].int())
    assert set(e.arenas) == held | {(2, 28, 46)}
    for a, b in zip(d, plain):
        assert torch.equal(a, b)
    again = m32.durations(text, tl.int(), mel, ml.int(), transient=True)   # an existing arena stays
    assert (2, 17, 23) in e.arenas and int(again.durations.sum()) == int(ml.sum())
