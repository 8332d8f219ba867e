"""CPU: tt2.data.extract_durations(method=...) driven by a stub model: "monotonic" goes through
monotonic_durations() and adds its manifest fields; "argmax" is byte for byte the default."""
import json
import os

import numpy as np
import pytest
import torch

from tt2.data import extract_durations
from tt2.model import AlignmentStats, Durations, MonotonicAlignment

L, H = 2, 2
LENS = {1: (5, 20), 2: (7, 11), 3: (6, 4), 4: (3, 30)}   # id -> (text_len, mel_len); utterance 3 has Ty < Tx


class StubModel:
    """durations(): frame n on phoneme (3 n) % text_len (not monotone).  monotonic_durations(): the
    even monotone spread floor(n * Te / Ty) and logp = -id / 10."""

    def __init__(self):
        self.calls = []

    def _head(self, text, head):
        B = text.shape[0]
        hd = torch.tensor([[1, 0]] * B if head == "best" else [list(head)] * B, dtype=torch.int32)
        self._last = AlignmentStats(None, None, torch.full((L, B, H), 0.5), tuple(range(L)))
        return hd, torch.full((B,), 0.5)

    def durations(self, text, text_len, mel, mel_len, head="best", layers=None, transient=False):
        self.calls.append(("durations", head, transient))
        hd, fc = self._head(text, head)
        dur = torch.zeros(text.shape, dtype=torch.int32)
        for b in range(text.shape[0]):
            for n in range(int(mel_len[b])):
                dur[b, (3 * n) % int(text_len[b])] += 1
        return Durations(dur, hd, fc)

    def monotonic_durations(self, text, text_len, mel, mel_len, head="best", layers=None, transient=False):
        self.calls.append(("monotonic_durations", head, transient))
        hd, fc = self._head(text, head)
        B, Tx = text.shape
        dur = torch.zeros(B, Tx, dtype=torch.int32)
        path = torch.full((B, mel.shape[1]), -1, dtype=torch.int32)
        for b in range(B):
            ty, te = int(mel_len[b]), min(int(text_len[b]), int(mel_len[b]))
            for n in range(ty):
                path[b, n] = n * te // ty
                dur[b, n * te // ty] += 1
        return MonotonicAlignment(dur, path, hd, fc, -text[:, 0].float() / 10)

    def alignment_stats(self, layers=None):
        return self._last


def make_batches():
    out = []
    for group in ((1, 2), (3, 4)):
        B, Tx, Ty = len(group), max(LENS[i][0] for i in group), max(LENS[i][1] for i in group)
        text = torch.zeros(B, Tx, dtype=torch.long)
        text[:, 0] = torch.tensor(group)
        tl = torch.tensor([LENS[i][0] for i in group])
        ml = torch.tensor([LENS[i][1] for i in group])
        out.append(([f"utt{i}" for i in group], text, tl, torch.zeros(B, Ty, 80), ml))
    return out


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_monotonic_writes_files_and_extra_fields(tmp_path):
    m = StubModel()
    out = str(tmp_path / "m")
    man = extract_durations(m, make_batches(), out, method="monotonic")
    assert json.load(open(os.path.join(out, "durations.json"))) == man
    assert man["method"] == "monotonic" and man["head"] == "best"
    assert m.calls == [("monotonic_durations", "best", True)] * 2
    for i, (tx, ty) in LENS.items():
        d = np.load(os.path.join(out, f"utt{i}.npy"))
        assert d.dtype == np.int32 and d.shape == (tx,) and int(d.sum()) == ty
        u = man["utterances"][f"utt{i}"]
        assert u["frames"] == ty and u["phonemes"] == tx and (u["layer"], u["head"]) == (1, 0)
        assert u["logp"] == pytest.approx(-i / 10)
        assert u["min_duration"] == int(d.min()) and (u["min_duration"] == 0) == (ty < tx)
    # a fixed head and the dataset pass reach monotonic_durations too; the choosing pass is unchanged
    m = StubModel()
    extract_durations(m, make_batches(), str(tmp_path / "f"), head=(0, 1), method="monotonic")
    assert m.calls == [("monotonic_durations", (0, 1), True)] * 2
    m = StubModel()
    man = extract_durations(m, make_batches(), str(tmp_path / "g"), head="dataset", method="monotonic")
    assert [c[0] for c in m.calls] == ["durations"] * 2 + ["monotonic_durations"] * 2
    assert man["dataset_head"] == [0, 0] and m.calls[-1][1] == (0, 0)


def test_argmax_is_the_default_byte_for_byte(tmp_path):
    a, b = StubModel(), StubModel()
    extract_durations(a, make_batches(), str(tmp_path / "a"))
    extract_durations(b, make_batches(), str(tmp_path / "b"), method="argmax")
    assert a.calls == b.calls == [("durations", "best", True)] * 2
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b"))
    for name in os.listdir(tmp_path / "a"):
        assert read(tmp_path / "a" / name) == read(tmp_path / "b" / name), name
    man = json.load(open(tmp_path / "a" / "durations.json"))
    assert "method" not in man and all("logp" not in u and "min_duration" not in u for u in man["utterances"].values())
    with pytest.raises(ValueError, match="method"):
        extract_durations(a, make_batches(), str(tmp_path / "c"), method="viterbi")
