"""tt2.audio.LoudnessNormalizer and its paths through tt2.data (GPU): measuring what it normalised,
the peak ceiling, unmeasured utterances, the chain behind a trimmer and a resampler,
collate(resampler=normalizer), MelExtractor left as it was, and the ownership of scratch and results.
The numbers themselves are held in tests/test_gpu_loudness_kernels.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _loudness_refs as R  # noqa: E402
from tt2 import audio, data  # noqa: E402

bits = R.bits


def levels(B=5, L=30000, seed=0):
    """Noise at levels 8 dB apart, ragged; utterance 3 is 0.3 s long (unmeasured), utterance 4 is
    quiet but for one loud sample (peak-limited)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, L)) * (0.2 * 10.0 ** (-8.0 * np.arange(B) / 20.0))[:, None]
    lens = [L, L - 4001, L - 1, 6600, L - 1500][:B]
    if B > 4:
        x[4, 7000] = 0.97
    return x.astype(np.float32), lens


def test_measure_after_normalize_lands_on_the_target():
    x, lens = levels()
    nz = audio.LoudnessNormalizer()
    ref = R.reference(x, lens, n_out=x.shape[1], **R.default_params())
    # no block changes sides of the absolute gate under the gain that is applied (so the gated set,
    # and with it the loudness, moves by the gain alone)
    for b, (E, pa, both) in enumerate(ref["gates"]):
        g2 = float(ref["gain"][b]) ** 2
        assert np.array_equal(E * g2 > nz.abs_sum, pa), b
    # (f32(gain * peak) can round one ulp past the ceiling in general; on this input it does not)
    assert np.abs(ref["y"][4]).max() <= np.float32(nz.ceiling)
    out = nz.normalize(torch.from_numpy(x).cuda(), torch.tensor(lens).cuda())
    assert isinstance(out, audio.Normalized) and out.audio.shape == x.shape and out.audio.dtype == torch.float32
    assert out.lens.dtype == torch.int32 and out.lens.tolist() == lens and out.limited.dtype == torch.int32
    assert out.limited.tolist() == ref["limited"].tolist() == [0, 0, 0, 0, 1]
    assert np.array_equal(bits(out.peak.cpu().numpy()), bits(ref["peak"]))
    assert np.abs(out.loud.cpu().numpy()[[0, 1, 2, 4]] - ref["loud"][[0, 1, 2, 4]]).max() < 1e-5
    after = nz.measure(out.audio, out.lens)
    assert isinstance(after, audio.Loudness) and after.energy.shape == (5, x.shape[1] // 2205 + 1)
    la = after.loud.cpu().numpy()
    print("after - target:", (la[:3] + 23.0).tolist())
    assert np.abs(la[:3] + 23.0).max() < 1e-3
    # the peak-limited one: below the target, its peak on the ceiling
    y = out.audio.cpu().numpy()
    assert la[4] < -23.5 and np.abs(y[4]).max() <= nz.ceiling and np.abs(y[4]).max() > 0.999 * nz.ceiling
    assert float(after.peak[4]) == np.abs(y[4]).max()
    # the unmeasured one comes back bit for bit; zeros past every length
    assert np.isneginf(out.loud.cpu().numpy()[3]) and float(out.gain[3]) == 1.0
    assert np.array_equal(bits(y[3, :lens[3]]), bits(x[3, :lens[3]]))
    for b, n in enumerate(lens):
        assert not y[b, n:].any() and np.array_equal(bits(y[b, :n]), bits(out.gain.cpu().numpy()[b] * x[b, :n]))
    # lens None, a CPU input, a strided view; __call__ is the first two fields
    a, n = nz(torch.from_numpy(x))
    full = R.reference(x, None, n_out=x.shape[1], **R.default_params())
    assert n.tolist() == [x.shape[1]] * 5 and np.abs(a.cpu().numpy() - full["y"]).max() < 1e-6
    wide = torch.zeros(5, x.shape[1] + 13, device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    a2, n2 = nz(wide[:, :x.shape[1]])
    assert torch.equal(a2, a) and torch.equal(n2, n)


def test_zero_size_batches():
    nz = audio.LoudnessNormalizer()
    e = nz.normalize(torch.zeros(0, 100))
    assert e.audio.shape == (0, 100) and e.lens.shape == (0,) and e.gain.shape == (0,) and e.limited.dtype == torch.int32
    e = nz.normalize(torch.zeros(2, 0))
    assert e.audio.shape == (2, 0) and e.lens.tolist() == [0, 0] and e.gain.tolist() == [1.0, 1.0]
    assert torch.isneginf(e.loud).all() and e.limited.tolist() == [0, 0] and e.peak.tolist() == [0.0, 0.0]
    m = nz.measure(torch.zeros(0, 5000))
    assert m.loud.shape == (0,) and m.energy.shape == (0, 3)
    m = nz.measure(torch.zeros(3, 0))
    assert torch.isneginf(m.loud).all() and m.energy.shape == (3, 1) and not m.energy.any()
    assert nz._ws.buf is None                                        # nothing was launched


def test_the_chain_equals_the_three_objects_called_in_turn():
    rs = audio.Resampler(48000)
    tr = audio.SilenceTrimmer(top_db=40, resampler=rs)
    chain = audio.LoudnessNormalizer(resampler=tr)
    alone_tr, alone_nz = audio.SilenceTrimmer(top_db=40), audio.LoudnessNormalizer()
    assert (chain.sr_in, chain.sr_out) == (48000, 22050)
    rng = np.random.default_rng(3)
    L = 70000
    x = 1e-4 * rng.normal(size=(3, L))
    x[:, 9000:60000] += (0.3 * np.sin(2 * np.pi * 300 * np.arange(51000) / 48000))[None] * np.array([1.0, 0.3, 0.05])[:, None]
    xd = torch.from_numpy(x.astype(np.float32)).cuda()
    lens = torch.tensor([L, L - 7000, 65000], dtype=torch.int32, device="cuda")
    got = chain.normalize(xd, lens)
    mid, ml = rs(xd, lens)
    mid, ml = alone_tr(mid, ml)
    want = alone_nz.normalize(mid, ml)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert torch.isfinite(got.loud).all() and all(0 < n < 30000 for n in got.lens.tolist())
    a, n = chain(xd, lens)
    assert torch.equal(a, want.audio) and torch.equal(n, want.lens)
    with pytest.raises(ValueError):
        audio.LoudnessNormalizer(resampler=audio.Resampler(48000, 16000))


def test_collate_with_a_normalizer_in_the_resampler_hook(tmp_path):
    from test_data_loudness import level_corpus
    root, sigs = level_corpus(str(tmp_path / "c"), n=2)
    ds = data.LJSpeech(root)
    nz = audio.LoudnessNormalizer()
    mx = audio.MelExtractor()
    idx = [1, 0]
    text, tl, mel, ml = data.collate(ds, idx, mx, resampler=nz)
    wavs = [ds.wav(i) for i in idx]
    L = max(len(w) for w in wavs)
    batch = np.zeros((2, L), dtype=np.float32)
    for b, w in enumerate(wavs):
        batch[b, :len(w)] = w
    lens = [len(w) for w in wavs]
    y, n = nz(torch.from_numpy(batch).cuda(), torch.tensor(lens).cuda())
    mel2, fr2 = mx(y, n)
    assert torch.equal(mel, mel2) and torch.equal(ml, fr2.to(torch.long)) and ml.tolist() == [1 + v // 256 for v in lens]
    # the two utterances were 12 dB apart; their mels' mean log energies now agree within 0.2 (1 dB is 0.115)
    m = [float(mel[b, :ml[b]].mean()) for b in range(2)]
    raw = data.collate(ds, idx, mx)[2]
    r = [float(raw[b, :ml[b]].mean()) for b in range(2)]
    print("mel means:", m, r)
    assert abs(m[0] - m[1]) < 0.2 and abs(abs(r[0] - r[1]) - 12 * np.log(10) / 20) < 0.3
    with pytest.raises(ValueError):
        data.collate(ds, idx, mx, resampler=audio.LoudnessNormalizer(resampler=audio.Resampler(48000)))


def test_normalize_corpus_on_the_gpu(tmp_path):
    from scipy.io import wavfile
    from test_data_loudness import level_corpus
    root, sigs = level_corpus(str(tmp_path / "c"))
    nz = audio.LoudnessNormalizer()
    man = data.normalize_corpus(data.LJSpeech(root), str(tmp_path / "n"), nz, batch_size=2)
    assert man["normalizer"] == nz.params() and man["unmeasured"] == ["U002"] and man["stats"]["limited"] == 1
    p = R.default_params()
    for i, s in enumerate(sigs):
        u = man["utterances"][f"U{i:03d}"]
        ref = R.reference(s[None, :], None, n_out=len(s), **p)
        assert u["limited"] == bool(ref["limited"][0]) and u["peak_in"] == float(ref["peak"][0])
        if i != 2:
            assert abs(u["loudness_in"] - float(ref["loud"][0])) < 1e-5
        _, pcm = wavfile.read(str(tmp_path / "n" / "wavs" / f"U{i:03d}.wav"))
        want = np.rint(ref["y"][0].astype(np.float64) * 32768)
        assert len(pcm) == len(s) and np.abs(pcm - want).max() <= 1


def test_mel_extractor_is_as_it_was_and_scratch_is_owned():
    x, lens = levels(seed=5)
    xd, ld = torch.from_numpy(x).cuda(), torch.tensor(lens).cuda()
    mx = audio.MelExtractor()
    mel0, fr0 = mx(xd, ld)
    mel0, fr0 = mel0.clone(), fr0.clone()
    nz = audio.LoudnessNormalizer()
    assert nz._ws.buf is None
    first = nz.normalize(xd, ld)
    torch.cuda.synchronize()
    ws = nz._ws.buf.data_ptr()
    keep = [t.clone() for t in first]
    mel1, fr1 = mx(xd, ld)
    assert torch.equal(mel0, mel1) and torch.equal(fr0, fr1)
    x2, lens2 = levels(B=3, L=17000, seed=6)
    second = nz.normalize(torch.from_numpy(x2).cuda(), torch.tensor(lens2).cuda())
    third = nz.normalize(xd, ld)
    torch.cuda.synchronize()
    assert nz._ws.buf.data_ptr() == ws                      # one scratch buffer, neither outgrown nor replaced
    for a, b, c in zip(first, keep, third):
        assert torch.equal(a, b) and torch.equal(a, c) and a.data_ptr() != c.data_ptr()
    assert second.audio.shape == (3, 17000) and second.audio.data_ptr() != first.audio.data_ptr()
    assert first.audio.data_ptr() != xd.data_ptr() and first.lens.data_ptr() != ld.data_ptr()
    other = audio.LoudnessNormalizer()
    other.measure(torch.zeros(1, 9000, device="cuda"))
    assert other._ws.buf.data_ptr() != nz._ws.buf.data_ptr()
