"""CPU: tt2.data.extract_durations driven by a stub model -- the files, their lengths, the
manifest, and the "dataset" pass' frame-weighted choice of one head."""
import json
import os

import numpy as np
import pytest
import torch

from tt2.data import extract_durations
from tt2.model import AlignmentStats, Durations

L, H = 2, 3


class StubModel:
    """durations() / alignment_stats() of a model whose head (l, h) puts frame n of an utterance on
    phoneme (n * (1 + l * H + h)) % text_len, with a focus rate given per (utterance, l, h)."""

    def __init__(self, focus_of):
        self.focus_of = focus_of   # ids -> [L, H] focus
        self.calls = []
        self.shapes = []   # (B, Tx, Ty) of every durations() call
        self.transient = []
        self._last = None

    def durations(self, text, text_len, mel, mel_len, head="best", layers=None, transient=False):
        B, Tx = text.shape
        ids = [int(x) for x in text[:, 0]]   # (the stub's batches carry the utterance id in text[:, 0])
        focus = torch.stack([self.focus_of[i] for i in ids], 1)   # [L, B, H]
        self._last = AlignmentStats(None, None, focus, tuple(range(L)))
        self.calls.append(head)
        self.shapes.append((B, Tx, mel.shape[1]))
        self.transient.append(transient)
        dur = torch.zeros(B, Tx, dtype=torch.int32)
        hd = torch.zeros(B, 2, dtype=torch.int32)
        fc = torch.zeros(B)
        for b in range(B):
            if head == "best":
                flat = int(torch.argmax(focus[:, b].reshape(-1)))
                l, h = flat // H, flat % H
            else:
                l, h = head
            for n in range(int(mel_len[b])):
                dur[b, (n * (1 + l * H + h)) % int(text_len[b])] += 1
            hd[b] = torch.tensor([l, h])
            fc[b] = focus[l, b, h]
        return Durations(dur, hd, fc)

    def alignment_stats(self, layers=None):
        return self._last


def make_batches():
    # utterance ids 1..5 in two batches; (text_len, mel_len) per utterance
    lens = {1: (5, 20), 2: (7, 11), 3: (4, 100), 4: (6, 9), 5: (3, 30)}
    out = []
    for group in ((1, 2, 3), (4, 5)):
        B, Tx, Ty = len(group), max(lens[i][0] for i in group), max(lens[i][1] for i in group)
        text = torch.zeros(B, Tx, dtype=torch.long)
        text[:, 0] = torch.tensor(group)
        tl = torch.tensor([lens[i][0] for i in group])
        ml = torch.tensor([lens[i][1] for i in group])
        out.append(([f"utt{i}" for i in group], text, tl, torch.zeros(B, Ty, 80), ml))
    return out, lens


def focus_table():
    g = torch.Generator().manual_seed(0)
    f = {i: torch.rand(L, H, generator=g) * 0.5 for i in range(1, 6)}
    f[3][1, 2], f[3][0, 1] = 0.9, 0.1   # the long utterance (100 of 170 frames) favours head (1, 2) ...
    for i in (1, 2, 4, 5):
        f[i][0, 1] = 0.8   # ... every other utterance head (0, 1): frame-weighted, (1, 2) still wins
        f[i][1, 2] = 0.5
    return f


def check_files(out_dir, batches, lens, manifest):
    assert json.load(open(os.path.join(out_dir, "durations.json"))) == manifest
    for ids, *_ in batches:
        for uid in ids:
            i = int(uid[3:])
            d = np.load(os.path.join(out_dir, f"{uid}.npy"))
            assert d.dtype == np.int32 and d.shape == (lens[i][0],)
            assert int(d.sum()) == lens[i][1]
            u = manifest["utterances"][uid]
            assert u["frames"] == lens[i][1] and u["phonemes"] == lens[i][0]
    assert set(manifest["utterances"]) == {f"utt{i}" for i in lens}


def test_best_head_per_utterance(tmp_path):
    batches, lens = make_batches()
    f = focus_table()
    m = StubModel(f)
    man = extract_durations(m, batches, str(tmp_path / "d"))
    check_files(str(tmp_path / "d"), batches, lens, man)
    assert man["head"] == "best" and m.calls == ["best", "best"]
    for i in lens:
        u = man["utterances"][f"utt{i}"]
        flat = int(torch.argmax(f[i].reshape(-1)))
        assert (u["layer"], u["head"]) == (flat // H, flat % H)
        assert u["focus"] == pytest.approx(float(f[i].reshape(-1)[flat]))


def test_fixed_head(tmp_path):
    batches, lens = make_batches()
    m = StubModel(focus_table())
    man = extract_durations(m, iter(batches), str(tmp_path / "d"), head=(1, 0))   # one pass: an iterator will do
    check_files(str(tmp_path / "d"), batches, lens, man)
    assert man["head"] == [1, 0] and m.calls == [(1, 0), (1, 0)]
    assert all((u["layer"], u["head"]) == (1, 0) for u in man["utterances"].values())
    d = np.load(str(tmp_path / "d" / "utt2.npy"))   # head (1, 0): frame n -> phoneme (4 n) % 7
    want = np.bincount([(4 * n) % 7 for n in range(11)], minlength=7)
    assert (d == want).all()


def test_dataset_pass_picks_the_frame_weighted_best_head(tmp_path):
    batches, lens = make_batches()
    f = focus_table()
    m = StubModel(f)
    man = extract_durations(m, batches, str(tmp_path / "d"), head="dataset")
    check_files(str(tmp_path / "d"), batches, lens, man)
    frames = sum(v[1] for v in lens.values())
    score = sum(f[i].double() * lens[i][1] for i in lens) / frames
    flat = int(torch.argmax(score.reshape(-1)))
    assert (flat // H, flat % H) == (1, 2)
    # unweighted, head (0, 1) would have won: the weighting is what picks (1, 2)
    assert int(torch.argmax(sum(f[i] for i in lens).reshape(-1))) == 0 * H + 1
    assert man["head"] == "dataset" and man["dataset_head"] == [1, 2]
    assert man["dataset_focus"] == pytest.approx(float(score[1, 2]))
    assert m.calls == ["best", "best", (1, 2), (1, 2)]
    assert all((u["layer"], u["head"]) == (1, 2) for u in man["utterances"].values())
    with pytest.raises(ValueError, match="twice"):
        extract_durations(m, iter(batches), str(tmp_path / "e"), head="dataset")


def test_ragged_batches_are_run_as_transient_shapes(tmp_path):
    """The engine keeps an arena per distinct (B, Tx, Ty) for good, and a corpus of ragged batches
    has one shape per batch: every durations() call asks for a transient arena, in both passes,
    and the batches reach the model as they are (padding would change the alignment)."""
    batches, lens = make_batches()
    m = StubModel(focus_table())
    extract_durations(m, batches, str(tmp_path / "d"), head="dataset")
    assert m.transient == [True] * 4
    assert m.shapes == [(3, 7, 100), (2, 6, 30)] * 2
