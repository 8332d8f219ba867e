"""Phoneme durations of an LJSpeech-format corpus from a trained model's alignment (GPU).

A thin command line over tt2.data.extract_durations: teacher-forced forwards of the checkpoint,
the fused alignment statistics (TransformerTTS.durations), one <id>.npy (int32 [text_len]) per
utterance and a durations.json manifest in --out.  The durations are the training targets of a
non-autoregressive student (the FastSpeech teacher procedure).

    python tools/extract_durations.py --data /data/LJSpeech-1.1 --checkpoint train.pt --out durations/ \
        [--head best | dataset | L,H] [--method argmax | monotonic] [--batch 16] [--dtype bf16] [--limit N]

Every batch has its own (B, Tx, Ty); extract_durations runs each as a transient shape, so the
engine does not keep an arena of activations per batch.

--checkpoint: a TransformerTTS.save_checkpoint file, or a plain state_dict saved with torch.save.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-tacotron2_amd"))
import torch  # noqa: E402


def parse_head(s: str):
    if s in ("best", "dataset"):
        return s
    l, h = s.split(",")
    return int(l), int(h)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="LJSpeech root (metadata.csv, wavs/)")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--head", type=parse_head, default="best", help='"best" (per utterance), "dataset" or "L,H"')
    ap.add_argument("--method", choices=("argmax", "monotonic"), default="argmax",
                    help="argmax histogram (TransformerTTS.durations) or monotonic alignment search "
                         "(TransformerTTS.monotonic_durations)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--limit", type=int, default=0, help="only the first N utterances (0: all)")
    a = ap.parse_args()

    from tt2.audio import MelExtractor
    from tt2.config import TTSConfig
    from tt2.data import LJSpeech, bucket_batches, collate, extract_durations
    from tt2.model import TransformerTTS

    model = TransformerTTS(TTSConfig(), dtype=torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    ck = torch.load(a.checkpoint, map_location="cpu", weights_only=True)
    if isinstance(ck, dict) and ck.get("format") == "tt2-train-1":
        model.load_checkpoint(a.checkpoint)
    else:
        model.load_state_dict(ck)
    ds, mx = LJSpeech(a.data), MelExtractor()
    n = min(len(ds), a.limit) if a.limit else len(ds)
    index_batches = bucket_batches([len(ds.items[i][1]) for i in range(n)], a.batch)

    class Batches:   # re-iterable (head="dataset" reads the corpus twice); one batch resident at a time
        def __iter__(self):
            for idx in index_batches:
                text, text_len, mel, mel_len = collate(ds, idx, mx)
                yield [ds.items[i][0] for i in idx], text, text_len.int(), mel, mel_len.int()

    man = extract_durations(model, Batches(), a.out, head=a.head, method=a.method)
    print(json.dumps({"out": a.out, "utterances": len(man["utterances"]), "head": man["head"],
                      "dataset_head": man.get("dataset_head"),
                      "mean_focus": sum(u["focus"] for u in man["utterances"].values()) / max(1, len(man["utterances"]))}))


if __name__ == "__main__":
    main()
