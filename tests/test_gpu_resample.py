"""tt2.audio.Resampler and its paths through tt2.data (GPU): against the float64 reference of
tests/_resample_refs.py fed the f32 bank the Resampler uploads, within the f32 evaluation bound
E[n] = (K + 2) 2^-24 sum_k |bank x| derived there; an analytic sum of tones; collate(resampler=);
the resampler's buffers against MelExtractor's; the corpus round trip.

Measured (MI355X): Resampler outputs at most 0.070 (48000), 0.085 (44100), 0.117 (24000) and 0.116
(16000) of E[n] from the reference; the sum of tones 8.9e-7 from the analytic signal where the
float64 reference itself is 8.2e-7 from it (E up to 8.1e-6)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _resample_refs as R  # noqa: E402
from tt2 import audio, data  # noqa: E402

bits = R.bits


@pytest.fixture(scope="module")
def rs48():
    return audio.Resampler(48000)


def bank32(rs):
    return rs.bank.taps.float().numpy()


def within_bound(y, out_lens, x, lens, rs):
    """Every valid output within E[n] of the float64 reference; zeros after; -> worst err / E."""
    bank, worst = bank32(rs), 0.0
    for b in range(x.shape[0]):
        ob = R.out_len(lens[b], rs.up, rs.down)
        assert int(out_lens[b]) == ob
        ref = R.resample(x[b], lens[b], bank, rs.up, rs.down, rs.half)
        E = R.bound(x[b], lens[b], bank, rs.up, rs.down, rs.half)
        err = np.abs(y[b, :ob].astype(np.float64) - ref)
        assert (err <= E).all(), (b, float((err / np.maximum(E, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(E, 1e-300)).max()))
        assert not y[b, ob:].any()
    return worst


@pytest.mark.parametrize("sr_in", [48000, 44100, 24000, 16000])
def test_resampler_against_the_reference(sr_in):
    rs = audio.Resampler(sr_in)
    B, L = 3, 9000
    x = (0.3 * np.random.default_rng(sr_in % 89).normal(size=(B, L))).astype(np.float32)
    lens = [L, 4321, 600]
    y, ol = rs(torch.from_numpy(x).cuda(), torch.tensor(lens).cuda())
    assert y.shape == (B, R.out_len(L, rs.up, rs.down)) and y.dtype == torch.float32 and y.is_cuda
    assert ol.dtype == torch.int32 and ol.shape == (B,)
    worst = within_bound(y.cpu().numpy(), ol.cpu().numpy(), x, lens, rs)
    print(f"{sr_in} -> 22050: worst error {worst:.3f} of E[n]")
    # lens None: every row is L long; fresh tensors on every call; a CPU input is uploaded
    y2, ol2 = rs(torch.from_numpy(x))
    assert ol2.tolist() == [y.shape[1]] * B and y2.data_ptr() != y.data_ptr()
    within_bound(y2.cpu().numpy(), ol2.cpu().numpy(), x, [L] * B, rs)
    y3, _ = rs(torch.from_numpy(x).cuda(), torch.tensor(lens).cuda())
    assert torch.equal(y3, y) and y3.data_ptr() != y.data_ptr()
    # a strided view of a wider buffer
    wide = torch.zeros(B, L + 13, device="cuda")
    wide[:, :L] = torch.from_numpy(x).cuda()
    y4, _ = rs(wide[:, :L], torch.tensor(lens).cuda())
    assert torch.equal(y4, y)


def test_identity_returns_its_inputs():
    rs = audio.Resampler(22050)
    x = torch.randn(2, 1000, device="cuda")
    lens = torch.tensor([1000, 10], dtype=torch.int32, device="cuda")
    y, ol = rs(x, lens)
    assert y is x and ol is lens
    y, ol = rs(x)
    assert y is x and ol.dtype == torch.int32 and ol.tolist() == [1000, 1000] and ol.device == x.device


def test_sum_of_tones_against_the_analytic_signal(rs48):
    """Tones below 0.7 of the new Nyquist (7717 Hz), sampled at 48 kHz and resampled, against the
    same tones sampled at 22.05 kHz, on the interior outputs (more than `half` input samples from
    either end).  Bar: 2 x the float64 reference's own error on this signal, plus E[n]."""
    freqs, amps, phases = [220.0, 1000.0, 3300.0, 5500.0, 7000.0], [0.3, 0.2, 0.15, 0.1, 0.1], [0.1, 0.7, 1.3, 2.1, 2.9]
    assert max(freqs) < 0.7 * 11025
    n_in = 12000
    x = R.tones(freqs, amps, phases, 48000, n_in).astype(np.float32)
    y, ol = rs48(torch.from_numpy(x)[None].cuda())
    n_out = R.out_len(n_in, 147, 320)
    assert ol.tolist() == [n_out]
    n = np.arange(n_out)
    i0 = n * 320 // 147
    idx = n[(i0 > rs48.half) & (i0 < n_in - 1 - rs48.half)]
    assert len(idx) > 5000
    want = R.tones(freqs, amps, phases, 22050, n_out)[idx]
    ref = R.resample(x, n_in, bank32(rs48), 147, 320, rs48.half, idx)
    E = R.bound(x, n_in, bank32(rs48), 147, 320, rs48.half, idx)
    own = float(np.abs(ref - want).max())
    got = np.abs(y[0].cpu().numpy()[idx].astype(np.float64) - want)
    print(f"tones: kernel {got.max():.3e}, float64 reference {own:.3e}, E up to {E.max():.3e}")
    # the design, by linearity: every tone is below 0.726 of the new Nyquist, where a unit tone is held
    # to 2 x 5.138e-6 (tests/test_resample_refs.py), plus the rounding of x to f32 (2^-25 per sample of
    # magnitude below 1) and of the bank to f32 through rows whose absolute sum is below 4
    assert float(np.abs(bank32(rs48)).sum(axis=1).max()) < 4
    assert own <= sum(amps) * 2 * 5.138e-6 + 2 * 4 * 2.0 ** -25
    assert (got <= 2 * own + E).all()


def _corpus(tmp_path, sr=48000, n=3):
    from test_data_resample import mini_corpus
    root, sigs = mini_corpus(str(tmp_path / f"c{sr}"), sr, n=n)
    return data.LJSpeech(root, sr=sr), sigs


def test_collate_with_a_resampler(tmp_path, rs48):
    ds, sigs = _corpus(tmp_path)
    mx = audio.MelExtractor()
    idx = [2, 0, 1]
    text, tl, mel, ml = data.collate(ds, idx, mx, resampler=rs48)
    wavs = [ds.wav(i) for i in idx]
    L = max(len(w) for w in wavs)
    batch = torch.zeros(3, L)
    for b, w in enumerate(wavs):
        batch[b, :len(w)] = torch.from_numpy(w)
    lens = torch.tensor([len(w) for w in wavs], dtype=torch.int32)
    y, ol = rs48(batch.cuda(), lens.cuda())
    mel2, fr2 = mx(y, ol)
    assert torch.equal(mel, mel2) and torch.equal(ml, fr2.to(torch.long))
    assert ml.tolist() == [1 + R.out_len(len(w), 147, 320) // 256 for w in wavs]
    assert mel.shape == (3, 1 + R.out_len(L, 147, 320) // 256, 80)
    with pytest.raises(ValueError):
        data.collate(ds, idx, mx, resampler=audio.Resampler(44100))


def test_mels_do_not_change_when_a_resampler_runs_in_between(rs48):
    """The resampler owns its buffers: it shares none with the extractor's plans."""
    mx = audio.MelExtractor()
    x = (0.3 * torch.randn(2, 6000, generator=torch.Generator().manual_seed(4))).cuda()
    lens = torch.tensor([6000, 3500], dtype=torch.int32, device="cuda")
    mel0, fr0 = mx(x, lens)
    mel0 = mel0.clone()
    other = torch.randn(2, 13061, device="cuda")                 # 13061 * 147 / 320 rounds up to 6000
    y, _ = rs48(other)
    assert y.shape == (2, 6000)
    mel1, fr1 = mx(x, lens)
    assert torch.equal(mel0, mel1) and torch.equal(fr0, fr1)
    mel_y, _ = mx(y)                                             # the same plan, the resampler's output as input
    y_again, _ = rs48(other)
    mel2, _ = mx(x, lens)
    assert torch.equal(mel0, mel2) and torch.equal(y, y_again)
    assert torch.equal(mel_y, mx(y)[0])


def test_resample_corpus_round_trip(tmp_path, rs48):
    from scipy.io import wavfile
    ds, sigs = _corpus(tmp_path)
    out = str(tmp_path / "c22")
    man = data.resample_corpus(ds, out, rs48, batch_size=2)
    assert man["resampler"] == rs48.params() and man["resampler"]["half"] == 59
    ds2 = data.LJSpeech(out)
    assert len(ds2) == 3
    for i in range(3):
        w = ds.wav(i)
        y, ol = rs48(torch.from_numpy(w)[None].cuda())
        y = y[0].cpu().numpy()
        rate, pcm = wavfile.read(os.path.join(out, "wavs", ds.items[i][0] + ".wav"))
        assert rate == 22050 and len(pcm) == int(ol[0]) == R.out_len(len(w), 147, 320)
        # in a batch or alone the kernel gives the same bits, so the file is the rounding of y
        assert np.abs(ds2.wav(i).astype(np.float64) - y).max() <= 0.5 / 32768
        u = man["utterances"][ds.items[i][0]]
        assert u == {"samples_in": len(w), "samples_out": len(pcm), "clipped": 0}
