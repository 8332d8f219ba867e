"""CPU: tt2.data.pad_batch and the one corpus pass behind resample_corpus / trim_corpus / normalize_corpus:
stages that leave the same utterance empty must leave the same corpus behind.  No GPU: stubs."""
import os

import numpy as np
import torch

from test_data_trim import padded_corpus
from tt2 import data


def test_pad_batch():
    wavs = [np.arange(1, n + 1, dtype=np.float32) for n in (3, 0, 5)]
    audio, lens = data.pad_batch(wavs)
    assert audio.dtype == torch.float32 and tuple(audio.shape) == (3, 5)
    assert lens.dtype == torch.int32 and lens.tolist() == [3, 0, 5]
    assert audio.tolist() == [[1, 2, 3, 0, 0], [0, 0, 0, 0, 0], [1, 2, 3, 4, 5]]


class EmptyingStage:
    """Passes the audio through and leaves corpus utterance 1 with no samples; all three stage protocols."""
    sr_in = sr_out = 22050

    def __init__(self):
        self.seen = 0

    def params(self):
        return {}

    def _cut(self, audio, lens):
        out = lens.clone()
        for b in range(len(lens)):
            if self.seen + b == 1:
                out[b] = 0
        self.seen += len(lens)
        return audio, out

    __call__ = _cut

    def trim(self, audio, lens):
        y, out = self._cut(audio, lens)
        return y, out, torch.zeros_like(out), None

    def normalize(self, audio, lens):
        y, out = self._cut(audio, lens)
        B = len(lens)
        return y, out, torch.full((B,), -20.0), torch.ones(B), torch.full((B,), 0.5), torch.zeros(B, dtype=torch.int32)


def test_trim_and_normalize_corpus_share_one_metadata_rewrite(tmp_path):
    root, _ = padded_corpus(str(tmp_path / "c"), n=3)
    ds = data.LJSpeech(root)
    a, b = str(tmp_path / "trimmed"), str(tmp_path / "normalised")
    mt = data.trim_corpus(ds, a, EmptyingStage(), batch_size=2)
    mn = data.normalize_corpus(ds, b, EmptyingStage(), batch_size=2)
    assert mt["empty"] == mn["empty"] == ["U001"]
    meta = open(os.path.join(a, "metadata.csv"), "rb").read()
    assert meta == open(os.path.join(b, "metadata.csv"), "rb").read()
    src = open(os.path.join(root, "metadata.csv"), "rb").read().splitlines(keepends=True)
    assert meta == b"".join(ln for ln in src if not ln.startswith(b"U001|"))
    assert sorted(os.listdir(os.path.join(a, "wavs"))) == sorted(os.listdir(os.path.join(b, "wavs"))) \
        == ["U000.wav", "U002.wav"]
    for name in ("U000.wav", "U002.wav"):      # passed through by both: the same PCM16 files
        assert open(os.path.join(a, "wavs", name), "rb").read() == open(os.path.join(b, "wavs", name), "rb").read()
    # resample_corpus has no "empty" list: a zero-length utterance is written like the others
    c = str(tmp_path / "resampled")
    mr = data.resample_corpus(ds, c, EmptyingStage(), batch_size=2)
    assert "empty" not in mr and mr["utterances"]["U001"]["samples_out"] == 0
    assert sorted(os.listdir(os.path.join(c, "wavs"))) == ["U000.wav", "U001.wav", "U002.wav"]
    assert len(data.read_wav(os.path.join(c, "wavs", "U001.wav"))[0]) == 0
    assert open(os.path.join(c, "metadata.csv"), "rb").read() == b"".join(src)
