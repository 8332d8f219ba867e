"""tt2.evaluate (mfcc, mcd_dtw) against the float64 references of tests/_dtw_refs.py, and
TransformerTTS.evaluate against infer() followed by mcd_dtw (GPU).

mfcc: element-wise |y - y64| <= 2 (80 + 2) 2^-24 sum_m |x_m| |w_km|, the f32 dot-product bound
(the DCT is one f32 tt2_gemm with an f32-rounded basis; the audio path relies on that GEMM being
true f32).  mcd_dtw: against mcd_ref run on the GPU's own cepstra, within 2 gamma of
test_gpu_dtw_kernels.py (gamma = (Na + Nb + C / 2 + 3) 2^-24, C = 13)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _dtw_refs import dct_ref, mcd_ref  # noqa: E402
from tt2 import evaluate  # noqa: E402
from tt2.config import TTSConfig  # noqa: E402
from tt2.model import Evaluation, TransformerTTS  # noqa: E402

U = 2.0 ** -24


def logmels(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, 80, generator=g) * 2.0 - 5.0).cuda()


@pytest.mark.parametrize("n_coef", [13, 15, 5])
def test_mfcc_against_float64(n_coef):
    x = logmels(3, 37, n_coef)
    y = evaluate.mfcc(x, n_coef)
    assert tuple(y.shape) == (3, 37, 16) and y.dtype == torch.float32
    y = y.cpu().numpy().astype(np.float64)
    x64, w = x.cpu().numpy().astype(np.float64), dct_ref(80, n_coef)
    ref = x64 @ w.T
    bound = 2 * (80 + 2) * U * (np.abs(x64) @ np.abs(w).T)
    err = np.abs(y[..., :n_coef + 1] - ref)
    print(f"max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert (y[..., n_coef + 1:] == 0).all()
    w32 = evaluate.dct_basis(80, n_coef)
    assert w32.dtype == torch.float32 and np.abs(w32.numpy() - w).max() <= 2.0 ** -25   # float64, rounded once


def test_mcd_dtw_against_reference():
    hyp, ref = logmels(3, 70, 1), logmels(3, 90, 2)
    ref[0, :70] = hyp[0] + 0.1 * logmels(1, 70, 3)[0]   # one close pair
    hl, rl = torch.tensor([70, 41, 64]), torch.tensor([90, 90, 33])
    r = evaluate.mcd_dtw(hyp, hl, ref, rl, want_path=True)
    q = evaluate.mcd_dtw(hyp, hl, ref, rl)
    assert isinstance(r, evaluate.MCD) and q.path_hyp is None and q.path_ref is None
    assert torch.equal(r.mcd, q.mcd) and torch.equal(r.total, q.total) and torch.equal(r.length, q.length)
    ch, cr = evaluate.mfcc(hyp).cpu().numpy(), evaluate.mfcc(ref).cpu().numpy()
    for b in range(3):
        na, nb = int(hl[b]), int(rl[b])
        mcd, total, length = mcd_ref(ch[b, :na], cr[b, :nb])
        gamma = (na + nb + 13 / 2 + 3) * U
        print(f"utt {b}: mcd {float(r.mcd[b]):.5f} dB ref {mcd:.5f} length {int(r.length[b])} ref {length}")
        assert abs(float(r.total[b]) - total) <= 2 * gamma * total
        assert int(r.length[b]) == length    # (Gaussian data: no near-ties)
        assert abs(float(r.mcd[b]) - mcd) <= 2 * gamma * mcd
        L = int(r.length[b])
        assert (r.path_hyp[b, L:] == -1).all() and int(r.path_hyp[b, L - 1]) == na - 1 and int(r.path_ref[b, L - 1]) == nb - 1


def test_mcd_of_identical_mels_is_zero_and_empty_is_nan():
    x = logmels(2, 50, 4)
    r = evaluate.mcd_dtw(x, torch.tensor([50, 0]), x.clone(), torch.tensor([50, 20]))
    assert float(r.mcd[0]) == 0.0 and float(r.total[0]) == 0.0 and int(r.length[0]) == 50
    assert torch.isnan(r.mcd[1]) and int(r.length[1]) == 0 and float(r.total[1]) == 0.0
    e = evaluate.mcd_dtw(x[:, :0], None, x, None)   # no frame decoded at all
    assert torch.isnan(e.mcd).all() and (e.length == 0).all()


def batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(1, 80, (2, 12), generator=g)
    tl = torch.tensor([12, 9], dtype=torch.int32)
    text[1, 9:] = 0
    mel = torch.randn(2, 30, 80, generator=g) - 4.0
    ml = torch.tensor([30, 21], dtype=torch.int32)
    mel[1, 21:] = 0
    return text, tl, mel, ml


def test_evaluate_is_infer_then_mcd_dtw():
    text, tl, mel, ml = batch()
    pair = []
    for _ in range(2):
        m = TransformerTTS(TTSConfig(), dtype=torch.bfloat16, seed=3).train()
        m.configure_optimizer(lr=1e-3, warmup=10.0)
        m.set_seed(9)
        m.train_step(text, tl, mel, ml)   # (sizes the workspaces before the capture)
        run = m.capture_train_step(2, 12, 30)
        run(text, tl, mel, ml)
        pair.append((m, run))
    (m, run), (twin, twin_run) = pair
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    was_training = m.training

    ev = m.evaluate(text, tl, mel, ml, max_len=48)
    assert isinstance(ev, Evaluation)
    hyp, out_len = twin.infer(text, tl, 48, stop_threshold=0.5, prenet_dropout=False)
    r = evaluate.mcd_dtw(hyp.float(), out_len, mel.cuda(), ml.cuda())
    assert torch.equal(ev.mel_hyp, hyp) and torch.equal(ev.hyp_len, out_len)
    assert torch.equal(ev.length, r.length)
    assert torch.equal(ev.mcd.view(torch.int32), r.mcd.view(torch.int32))   # bit for bit, NaN included
    assert torch.equal(ev.ref_len.cpu(), ml)
    print("mcd", ev.mcd.tolist(), "length", ev.length.tolist(), "hyp_len", ev.hyp_len.tolist())

    assert m.training == was_training
    sd1 = m.state_dict()
    assert list(sd0) == list(sd1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    # the step captured beforehand still replays, to the loss of a twin that only ran infer()
    la = run(text, tl, mel, ml).clone()
    lb = twin_run(text, tl, mel, ml).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(la).all() and torch.equal(la, lb), (la, lb)
    # the default max_len: min(2 Ty, table rows - 1, the DTW frame limit) = 60 here
    ev2 = m.evaluate(text, tl, mel, ml)
    assert ev2.mel_hyp.shape[1] <= 60 and int(ev2.hyp_len.max()) <= 60
