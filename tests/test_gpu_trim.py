"""tt2.audio.SilenceTrimmer and its paths through tt2.data (GPU): against the float64 reference of
tests/_trim_refs.py on tone bursts within silence and low noise (every frame further from the
threshold than f32 can move it, which the test asserts first, so the float64 decision is the only
one), MelExtractor on its output, collate(resampler=trimmer), the resample-then-trim composite, and
the ownership of scratch and results."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _trim_refs as R  # noqa: E402
from tt2 import audio, data  # noqa: E402

bits = R.bits


def bursts(B=4, L=30000, noise=1e-4, seed=0):
    """Tone bursts (amplitude 0.3) at different places, one utterance with two, in noise of the given
    amplitude (0: exact silence); ragged lengths."""
    rng = np.random.default_rng(seed)
    x = noise * rng.normal(size=(B, L))
    t = np.arange(L) / 22050.0
    spans = [[(6000, 21000)], [(0, 9000)], [(12000, 30000)], [(5000, 9000), (16000, 22000)]]
    for b in range(B):
        for lo, hi in spans[b % 4]:
            x[b, lo:hi] += 0.3 * np.sin(2 * np.pi * (180 + 70 * b) * t[lo:hi] + 0.5)
    lens = [L, L - 4001, L - 1, L - 1500][:B]
    return x.astype(np.float32), lens


def against_reference(tr, x, lens, want_energy=True):
    for b in range(x.shape[0]):
        assert R.decision_margin(x[b], lens[b], tr.hop, tr.r, np.float32(tr.ratio)) > 0
    out = tr.trim(torch.from_numpy(x).cuda(), torch.tensor(lens).cuda(), want_energy=want_energy)
    ref = R.reference(x, lens, tr.hop, tr.r, tr.keep, np.float32(tr.ratio), x.shape[1])
    assert isinstance(out, audio.Trimmed) and out.audio.shape == x.shape and out.audio.dtype == torch.float32
    assert out.lens.dtype == torch.int32 and out.start.dtype == torch.int32 and out.audio.is_cuda
    assert out.lens.tolist() == ref[1] and out.start.tolist() == ref[2]
    assert np.array_equal(bits(out.audio.cpu().numpy()), bits(ref[0]))
    if want_energy:
        nf = x.shape[1] // tr.hop + 1
        assert out.energy.shape == (x.shape[0], nf)
        en = out.energy.cpu().numpy().astype(np.float64)
        for b in range(x.shape[0]):
            assert (np.abs(en[b] - ref[3][b]) <= R.energy_bound(x[b], lens[b], tr.hop, tr.r).max()).all()
    else:
        assert out.energy is None
    return out, ref


def test_trimmer_against_the_reference():
    x, lens = bursts()
    out, ref = against_reference(audio.SilenceTrimmer(top_db=40), x, lens)
    assert ref[2][1] == 0 and ref[2][0] > 4000 and ref[2][2] > 10000       # trimmed where there was silence
    assert ref[2][2] + ref[1][2] == lens[2] and ref[1][3] > 16000          # to the end; interior silence kept
    against_reference(audio.SilenceTrimmer(top_db=40, frame=1024, hop=256, keep=300), x, lens, want_energy=False)
    # the defaults on exact silence
    x0, lens0 = bursts(noise=0.0, seed=1)
    against_reference(audio.SilenceTrimmer(), x0, lens0)
    # lens None, a CPU input, a strided view; __call__ is the first two fields
    tr = audio.SilenceTrimmer(top_db=40)
    a, n = tr(torch.from_numpy(x))
    full = R.reference(x, None, tr.hop, tr.r, 0, np.float32(tr.ratio), x.shape[1])
    assert n.tolist() == full[1] and np.array_equal(bits(a.cpu().numpy()), bits(full[0]))
    wide = torch.zeros(4, x.shape[1] + 13, device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    a2, n2 = tr(wide[:, :x.shape[1]])
    assert torch.equal(a2, a) and torch.equal(n2, n)
    # nothing to trim from: empty results of the right shapes
    e = tr.trim(torch.zeros(0, 100), want_energy=True)
    assert e.audio.shape == (0, 100) and e.lens.shape == (0,) and e.energy.shape == (0, 1)
    e = tr.trim(torch.zeros(2, 0))
    assert e.audio.shape == (2, 0) and e.lens.tolist() == [0, 0] and e.start.tolist() == [0, 0]


def test_mels_of_the_trimmed_batch_equal_mels_of_the_host_sliced_audio():
    x, lens = bursts(seed=2)
    tr = audio.SilenceTrimmer(top_db=40)
    mx = audio.MelExtractor()
    y, ol = tr(torch.from_numpy(x).cuda(), torch.tensor(lens).cuda())
    mel, fr = mx(y, ol)
    ref = R.reference(x, lens, tr.hop, tr.r, 0, np.float32(tr.ratio), x.shape[1])
    host = np.zeros_like(x)
    for b in range(x.shape[0]):
        host[b, :ref[1][b]] = x[b, ref[2][b]:ref[2][b] + ref[1][b]]
    mel2, fr2 = mx(torch.from_numpy(host).cuda(), torch.tensor(ref[1], dtype=torch.int32).cuda())
    assert torch.equal(fr, fr2) and torch.equal(mel, mel2)
    assert fr.tolist() == [1 + n // 256 for n in ref[1]]


def _corpus(tmp_path, sr=22050):
    from test_data_trim import padded_corpus
    root, sigs = padded_corpus(str(tmp_path / f"c{sr}"), sr=sr, n=2)
    return data.LJSpeech(root, sr=sr), sigs


def test_collate_with_a_trimmer_in_the_resampler_hook(tmp_path):
    ds, sigs = _corpus(tmp_path)
    tr = audio.SilenceTrimmer(frame=256, hop=64)
    mx = audio.MelExtractor()
    idx = [1, 0]
    text, tl, mel, ml = data.collate(ds, idx, mx, resampler=tr)
    wavs = [ds.wav(i) for i in idx]
    L = max(len(w) for w in wavs)
    batch = np.zeros((2, L), dtype=np.float32)
    for b, w in enumerate(wavs):
        batch[b, :len(w)] = w
    lens = [len(w) for w in wavs]
    ref = R.reference(batch, lens, 64, 2, 0, np.float32(tr.ratio), L)
    assert all(0 < n < m - 700 for n, m in zip(ref[1], lens))                # of 1100 and 1320 samples of silence
    assert ml.tolist() == [1 + n // 256 for n in ref[1]]
    mel2, fr2 = mx(torch.from_numpy(ref[0].astype(np.float32)).cuda(), torch.tensor(ref[1], dtype=torch.int32).cuda())
    assert torch.equal(mel, mel2) and torch.equal(ml, fr2.to(torch.long))
    with pytest.raises(ValueError):
        data.collate(ds, idx, mx, resampler=audio.SilenceTrimmer(resampler=audio.Resampler(48000)))


def test_trim_corpus_on_the_gpu(tmp_path):
    from scipy.io import wavfile
    ds, sigs = _corpus(tmp_path)
    tr = audio.SilenceTrimmer(frame=256, hop=64, keep=32)
    man = data.trim_corpus(ds, str(tmp_path / "t"), tr, batch_size=2)
    assert man["trimmer"] == tr.params() and man["empty"] == []
    for i, s in enumerate(sigs):
        u = man["utterances"][f"U{i:03d}"]
        ref = R.reference(s[None, :], None, 64, 2, 32, np.float32(tr.ratio), len(s))
        assert (u["start"], u["samples_out"], u["samples_in"], u["clipped"]) == (ref[2][0], ref[1][0], len(s), 0)
        _, pcm = wavfile.read(str(tmp_path / "t" / "wavs" / f"U{i:03d}.wav"))
        assert np.array_equal(pcm, np.rint(s[u["start"]:u["start"] + u["samples_out"]] * 32768).astype(np.int16))


def test_resample_then_trim_in_one_object():
    rs = audio.Resampler(48000)
    both = audio.SilenceTrimmer(top_db=40, resampler=rs)
    alone = audio.SilenceTrimmer(top_db=40)
    assert (both.sr_in, both.sr_out) == (48000, 22050)
    rng = np.random.default_rng(3)
    L = 40000
    x = 1e-4 * rng.normal(size=(3, L))
    x[:, 9000:30000] += 0.3 * np.sin(2 * np.pi * 300 * np.arange(21000) / 48000)
    xd = torch.from_numpy(x.astype(np.float32)).cuda()
    lens = torch.tensor([L, L - 7000, 25000], dtype=torch.int32, device="cuda")
    got = both.trim(xd, lens, want_energy=True)
    mid, ml = rs(xd, lens)
    want = alone.trim(mid, ml, want_energy=True)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert all(0 < n < m for n, m in zip(got.lens.tolist(), ml.tolist())) and min(got.start.tolist()) > 3000
    a, n = both(xd, lens)
    assert torch.equal(a, want.audio) and torch.equal(n, want.lens)


def test_scratch_is_reused_and_results_are_fresh():
    tr = audio.SilenceTrimmer(top_db=40)
    assert tr._ws.buf is None
    x, lens = bursts(seed=5)
    first = tr.trim(torch.from_numpy(x).cuda(), torch.tensor(lens).cuda(), want_energy=True)
    torch.cuda.synchronize()
    ws = tr._ws.buf.data_ptr()
    keep = [t.clone() for t in first]
    x2, lens2 = bursts(B=3, L=17000, seed=6)
    second = tr.trim(torch.from_numpy(x2).cuda(), torch.tensor(lens2).cuda(), want_energy=True)
    third = tr.trim(torch.from_numpy(x).cuda(), torch.tensor(lens).cuda(), want_energy=True)
    torch.cuda.synchronize()
    assert tr._ws.buf.data_ptr() == ws                      # one scratch buffer, neither outgrown nor replaced
    for a, b, c in zip(first, keep, third):
        assert torch.equal(a, b) and torch.equal(a, c) and a.data_ptr() != c.data_ptr()
    assert second.audio.shape == (3, 17000) and second.audio.data_ptr() != first.audio.data_ptr()
    # a shape that outgrows it (a block sum per sample at hop 1) replaces it; results stand
    fine = audio.SilenceTrimmer(frame=2, hop=1)
    small = fine.trim(torch.ones(2, 1000, device="cuda"))
    torch.cuda.synchronize()
    before = fine._ws.buf.numel()
    large = fine.trim(torch.ones(8, 40000, device="cuda"))
    torch.cuda.synchronize()
    assert fine._ws.buf.numel() > before and fine._ws.buf.numel() >= 4 * 4 * 40000
    assert small.lens.tolist() == [1000, 1000] and large.lens.tolist() == [40000] * 8
    assert torch.equal(small.audio, torch.ones(2, 1000, device="cuda"))
    other = audio.SilenceTrimmer()
    other.trim(torch.zeros(1, 600, device="cuda"))
    assert other._ws.buf.data_ptr() != tr._ws.buf.data_ptr()
