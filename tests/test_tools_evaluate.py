"""CPU: tools/evaluate.py's argument parsing and the eval.json it writes, driven by a stub model
(test_data_mono.py's manner)."""
import importlib.util
import json
import math
import os
from types import SimpleNamespace

import pytest
import torch

from tt2.model import Evaluation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("tools_evaluate", os.path.join(ROOT, "tools", "evaluate.py"))
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

# id -> (ref_len, hyp_len, mcd): utterance 3 runs into max_len, utterance 4 decodes no frame
UTT = {1: (20, 22, 6.0), 2: (10, 9, 3.0), 3: (8, 16, 9.0), 4: (30, 0, float("nan"))}


class StubModel:
    cfg = SimpleNamespace(max_len=4096)

    def __init__(self):
        self.calls = []

    def evaluate(self, text, text_len, mel, mel_len, max_len=None, stop_threshold=0.5, prenet_dropout=False,
                 n_coef=13, want_path=False):
        self.calls.append((max_len, stop_threshold, n_coef))
        ids = text[:, 0].tolist()
        hyp = torch.tensor([UTT[i][1] for i in ids], dtype=torch.int32)
        mcd = torch.tensor([UTT[i][2] for i in ids])
        length = torch.tensor([max(UTT[i][0], UTT[i][1]) if UTT[i][1] else 0 for i in ids], dtype=torch.int32)
        return Evaluation(mcd, length, hyp, mel_len, torch.zeros(len(ids), int(hyp.max()), 80))


def make_batches():
    out = []
    for group in ((1, 2), (3, 4)):
        B, Ty = len(group), max(UTT[i][0] for i in group)
        text = torch.zeros(B, 5, dtype=torch.long)
        text[:, 0] = torch.tensor(group)
        ml = torch.tensor([UTT[i][0] for i in group], dtype=torch.int32)
        out.append(([f"utt{i}" for i in group], text, torch.full((B,), 5, dtype=torch.int32), torch.zeros(B, Ty, 80), ml))
    return out


def test_argument_parsing():
    a = tool.parse_args(["--data", "d", "--checkpoint", "c.pt", "--out", "o"])
    assert (a.data, a.checkpoint, a.out, a.batch, a.dtype, a.n_coef, a.stop_threshold, a.limit) == \
        ("d", "c.pt", "o", 16, "bf16", 13, 0.5, 0)
    a = tool.parse_args(["--data", "d", "--checkpoint", "c", "--out", "o", "--batch", "4", "--dtype", "f32",
                         "--n-coef", "12", "--stop-threshold", "0.4", "--limit", "7"])
    assert (a.batch, a.dtype, a.n_coef, a.stop_threshold, a.limit) == (4, "f32", 12, 0.4, 7)
    for bad in (["--out", "o"], ["--data", "d", "--checkpoint", "c", "--out", "o", "--n-coef", "16"],
                ["--data", "d", "--checkpoint", "c", "--out", "o", "--batch", "0"],
                ["--data", "d", "--checkpoint", "c", "--out", "o", "--dtype", "f16"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


def test_eval_json_schema(tmp_path):
    m = StubModel()
    out = str(tmp_path / "e")
    man = tool.evaluate_corpus(m, make_batches(), out, n_coef=12, stop_threshold=0.4)
    assert json.load(open(os.path.join(out, "eval.json"))) == man
    assert sorted(man) == ["failed", "max_len_factor", "mean_mcd", "n_coef", "scored", "utterances"]
    # max_len = min(2 Ty, table rows - 1, the DTW frame limit) per batch
    assert m.calls == [(40, 0.4, 12), (60, 0.4, 12)]
    assert sorted(man["utterances"]) == ["utt1", "utt2", "utt3", "utt4"]
    for i, (ref, hyp, mcd) in UTT.items():
        u = man["utterances"][f"utt{i}"]
        assert sorted(u) == ["hit_max_len", "hyp_len", "mcd", "path_length", "ref_len"]
        assert (u["ref_len"], u["hyp_len"]) == (ref, hyp)
        assert u["mcd"] == (None if math.isnan(mcd) else pytest.approx(mcd))
        assert u["path_length"] == (max(ref, hyp) if hyp else 0)
    assert [man["utterances"][f"utt{i}"]["hit_max_len"] for i in (1, 2, 3, 4)] == [False, False, False, False]
    assert man["failed"] == 1 and man["scored"] == 3 and man["n_coef"] == 12
    assert man["mean_mcd"] == pytest.approx((6.0 * 20 + 3.0 * 10 + 9.0 * 8) / 38)


def test_hit_max_len_is_not_scored(tmp_path):
    m = StubModel()
    m.cfg = SimpleNamespace(max_len=17)   # max_len = 16: utterance 3 (16 frames) and, in batch 1, utterance 1 hit it
    man = tool.evaluate_corpus(m, make_batches(), str(tmp_path / "e"))
    assert m.calls == [(16, 0.5, 13), (16, 0.5, 13)]
    hits = {k: u["hit_max_len"] for k, u in man["utterances"].items()}
    assert hits == {"utt1": True, "utt2": False, "utt3": True, "utt4": False}
    assert man["failed"] == 3 and man["scored"] == 1 and man["mean_mcd"] == pytest.approx(3.0)
