"""CPU: the command line of tools/extract_pitch.py with and without --track, and
tt2.data.extract_pitch with a stub tracker: the manifest names the tracker only when there is one."""
import importlib.util
import json
import os

import pytest
import torch

from tt2 import audio
from tt2.data import extract_pitch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool():
    spec = importlib.util.spec_from_file_location("extract_pitch_tool", os.path.join(ROOT, "tools", "extract_pitch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class NoMel:   # PitchExtractor only keeps it
    dev = "cpu"


class StubExtractor(audio.PitchExtractor):
    """A PitchExtractor without a device: a constant 200 Hz in every valid frame."""

    def __init__(self, extractor=None, **kw):
        super().__init__(NoMel(), **kw)

    def __call__(self, a, lens):
        B, L = a.shape
        frames = (1 + lens // 256).to(torch.int32)
        live = torch.arange(1 + L // 256)[None, :] < frames[:, None]
        f0 = torch.where(live, 200.0, 0.0)
        return audio.Pitch(f0, f0 > 0, torch.where(live, 0.05, 1.0), live.float(), frames)


class StubTracker(audio.PitchTracker):
    def track(self, a, lens):
        p = self.px(a, lens)
        return audio.PitchTrack(p, p.voiced.int() * 110, torch.zeros(a.shape[0]))


def corpus():
    return [(["u1", "u2"], torch.zeros(2, 256 * 5), torch.tensor([256 * 5, 256 * 3 + 7], dtype=torch.int32))]


def test_tool_defaults_without_track():
    a = tool().parse_args(["--data", "/d", "--out", "o"])
    assert (a.data, a.out, a.durations, a.batch, a.fmin, a.fmax, a.threshold, a.limit) == \
        ("/d", "o", None, 16, 65.0, 600.0, 0.1, 0)
    assert (a.track, a.jump, a.switch, a.unvoiced) == ("none", 1.0, 0.1, 0.2)
    a = tool().parse_args(["--data", "/d", "--out", "o", "--track", "viterbi", "--jump", "0.5", "--switch", "0.2",
                           "--unvoiced", "0.3"])
    assert (a.track, a.jump, a.switch, a.unvoiced) == ("viterbi", 0.5, 0.2, 0.3)
    with pytest.raises(SystemExit):
        tool().parse_args(["--data", "/d", "--out", "o", "--track", "median"])


def test_tool_builds_the_extractor_it_is_asked_for(monkeypatch):
    """Without --track the tool hands extract_pitch a plain PitchExtractor, as before: the same
    params(), hence the same pitch.json."""
    monkeypatch.setattr(audio, "PitchExtractor", StubExtractor)
    t = tool()
    px = t.make_extractor(t.parse_args(["--data", "/d", "--out", "o", "--fmin", "80"]))
    assert type(px) is StubExtractor and px.fmin == 80.0
    assert px.params() == {"sr": 22050, "hop": 256, "frame": 1024, "fmin": 80.0, "fmax": 600.0, "threshold": 0.1,
                           "tau_min": 37, "tau_max": 275}
    tr = t.make_extractor(t.parse_args(["--data", "/d", "--out", "o", "--track", "viterbi", "--jump", "2"]))
    assert type(tr) is audio.PitchTracker and type(tr.px) is StubExtractor
    assert (tr.jump, tr.switch, tr.unvoiced) == (2.0, 0.1, 0.2)


def test_manifest_names_the_tracker_only_when_there_is_one(tmp_path):
    plain, tracked = str(tmp_path / "plain"), str(tmp_path / "tracked")
    px = StubExtractor()
    man = extract_pitch(corpus(), plain, px)
    assert "track" not in man["extractor"] and man["extractor"] == px.params()
    assert not {"track", "jump", "switch", "unvoiced"} & set(json.load(open(os.path.join(plain, "pitch.json")))["extractor"])
    tr = StubTracker(px, jump=0.5)
    man = extract_pitch(corpus(), tracked, tr)
    on_disk = json.load(open(os.path.join(tracked, "pitch.json")))
    assert man == on_disk
    assert on_disk["extractor"] == {**px.params(), "track": "viterbi", "jump": 0.5, "switch": 0.1, "unvoiced": 0.2}
    assert sorted(os.listdir(tracked)) == sorted(os.listdir(plain))
    assert {k: v["frames"] for k, v in on_disk["utterances"].items()} == {"u1": 6, "u2": 4}
