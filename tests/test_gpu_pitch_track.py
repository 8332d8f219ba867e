"""tt2.audio.PitchTracker end to end (GPU): on the glide of tests/_pitch_track_refs.py, fed as a
waveform so that d' is the GPU's own, the tracker meets the conditions the references meet on the
CPU and a plain PitchExtractor does not; what it takes from tt2_yin is bit-identical to
PitchExtractor's; it leaves the shared plan buffer usable; ragged lengths, extract_pitch and f0_dtw
take it as they take an extractor.

The waveform is the glide's samples 512 .. L - 512: with the extractor's reflect padding of 512,
frame f is again centred on sample 256 f + 512 of the glide and only the first and last two frames
see reflected samples instead of the glide's own."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pitch_track_refs as R  # noqa: E402
from tt2 import audio, data, evaluate  # noqa: E402


@pytest.fixture(scope="module")
def mx():
    return audio.MelExtractor()


@pytest.fixture(scope="module")
def glide():
    x, truth = R.glide_signal()
    return torch.from_numpy(x[512:len(x) - 512].astype(np.float32))[None].cuda(), truth


def lags_of(p: audio.Pitch):
    """The (unrefined) lag of each voiced frame of a Pitch, 0 where unvoiced."""
    f0 = p.f0.double().cpu().numpy()
    return np.where(f0 > 0, np.rint(R.SR / np.where(f0 > 0, f0, 1.0)), 0).astype(np.int64)


def raw(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_tracker_follows_the_glide_where_the_extractor_does_not(mx, glide):
    wav, truth = glide
    px = audio.PitchExtractor(mx)
    tr = audio.PitchTracker(px)
    assert (tr.tau_min, tr.tau_max) == R.GLIDE_RANGE and tr.mx is mx
    t = tr.track(wav)
    lag = t.lag[0].cpu().numpy()
    assert t.lag.dtype == torch.int32 and tuple(t.lag.shape) == (1, R.GLIDE_T) and tuple(t.cost.shape) == (1,)
    assert R.glide_tracked_ok(lag, truth) == [], (lag, np.rint(truth))
    assert torch.equal(t.pitch.voiced, t.lag > 0) and torch.equal(t.pitch.voiced, t.pitch.f0 > 0)
    f0 = t.pitch.f0[0].cpu().numpy()
    v = lag > 0
    assert np.all(np.abs(R.SR / f0[v] - lag[v]) <= 0.5 + 1e-3)   # the refinement: |off| <= 1/2 where a > b and c >= b
    plain = px(wav)
    sel = lags_of(plain)[0]
    assert R.glide_tracked_ok(sel, truth) != []
    assert R.glide_octave_errors(sel, truth) >= 5, sel[20:28]
    # what the tracker takes from tt2_yin is what PitchExtractor returns, bit for bit
    for got, want in ((t.pitch.aperiodicity, plain.aperiodicity), (t.pitch.energy, plain.energy)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(t.pitch.frames, plain.frames) and t.pitch.frames.tolist() == [R.GLIDE_T]
    again = tr(wav)
    assert isinstance(again, audio.Pitch) and torch.equal(again.f0.view(torch.int32), t.pitch.f0.view(torch.int32))


def test_shared_plan_buffer_and_ragged_lengths(mx, glide):
    wav, _ = glide
    L = wav.shape[1]
    lens = [L, 9000, 700]
    batch = wav.repeat(3, 1).contiguous()
    batch[1] = batch[1].roll(-3000)
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    px = audio.PitchExtractor(mx)
    tr = audio.PitchTracker(px)
    mel0, fr0 = mx(batch, ld)
    p0 = px(batch, ld)
    t = tr.track(batch, ld)
    mel1, fr1 = mx(batch, ld)
    p1 = px(batch, ld)
    assert torch.equal(mel0.view(torch.int32), mel1.view(torch.int32)) and torch.equal(fr0, fr1)
    for a, b in zip(p0, p1):
        assert torch.equal(raw(a), raw(b))
    for got, want in ((t.pitch.aperiodicity, p0.aperiodicity), (t.pitch.energy, p0.energy)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert t.pitch.frames.tolist() == [1 + n // 256 for n in lens] and torch.equal(t.pitch.frames, p0.frames)
    for b, n in enumerate(lens):   # an utterance does not depend on its batch
        nf = 1 + n // 256
        alone = tr.track(batch[b:b + 1, :n].contiguous())
        assert torch.equal(alone.lag[0], t.lag[b, :nf]) and (t.lag[b, nf:] == -1).all()
        assert torch.equal(alone.pitch.f0[0].view(torch.int32), t.pitch.f0[b, :nf].view(torch.int32))
        assert (t.pitch.f0[b, nf:] == 0).all() and not t.pitch.voiced[b, nf:].any()
        assert torch.equal(alone.cost.view(torch.int32), t.cost[b:b + 1].view(torch.int32))
    assert (t.lag[1] > 0).any() and (t.lag[2] >= 0).sum() == 3


def test_extract_pitch_and_f0_dtw_take_a_tracker(mx, glide, tmp_path):
    wav, _ = glide
    L = wav.shape[1]
    tr = audio.PitchTracker(audio.PitchExtractor(mx), jump=0.5)
    lens = torch.tensor([L, 9000], dtype=torch.int32)
    out = str(tmp_path / "pitch")
    man = data.extract_pitch([(["g1", "g2"], wav.repeat(2, 1).cpu(), lens)], out, tr)
    assert man["extractor"] == tr.params() == json.load(open(os.path.join(out, "pitch.json")))["extractor"]
    assert {k: man["extractor"][k] for k in ("track", "jump", "switch", "unvoiced")} == \
        {"track": "viterbi", "jump": 0.5, "switch": 0.1, "unvoiced": 0.2}
    assert sorted(os.listdir(out)) == sorted(["pitch.json", "g1.f0.npy", "g1.energy.npy", "g2.f0.npy", "g2.energy.npy"])
    p = tr(wav.repeat(2, 1), lens.cuda())
    for b, uid in enumerate(("g1", "g2")):
        n = int(p.frames[b])
        assert np.array_equal(np.load(os.path.join(out, f"{uid}.f0.npy")), p.f0[b, :n].cpu().numpy())
    both = wav.repeat(2, 1).contiguous()
    s, m = evaluate.f0_dtw(both, lens.cuda(), both.clone(), lens.cuda(), pitch=audio.PitchTracker(audio.PitchExtractor(mx)))
    assert s.rmse_cents.tolist() == [0, 0] and s.vuv_error.tolist() == [0, 0] and s.gpe.tolist() == [0, 0]
    assert m.total.tolist() == [0, 0] and (s.voiced_pairs > 0).all()
