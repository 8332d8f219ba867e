"""MCD-DTW of a trained model's free-running decode over an LJSpeech-format corpus (GPU).

A thin command line over TransformerTTS.evaluate: each batch is decoded autoregressively from its
text and scored against its ground-truth mels (mel-cepstral distortion along the dynamic-time-
warping path, tt2.evaluate).  Writes eval.json in --out:

    {"utterances": {id: {"mcd", "hyp_len", "ref_len", "path_length", "hit_max_len"}},
     "mean_mcd":  the mean over the scored utterances weighted by their reference frames,
     "scored", "failed": utterances scored / that hit max_len or produced no frame (not scored),
     "n_coef", "max_len_factor"}

    python tools/evaluate.py --data /data/LJSpeech-1.1 --checkpoint train.pt --out eval/ \
        [--batch 16] [--dtype bf16] [--n-coef 13] [--stop-threshold 0.5] [--limit N]

--checkpoint: a TransformerTTS.save_checkpoint file, or a plain state_dict saved with torch.save.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-tacotron2_amd"))
import torch  # noqa: E402

DTW_MAX_FRAMES = 2048   # TT2_DTW_MAX_FRAMES


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="LJSpeech root (metadata.csv, wavs/)")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--n-coef", type=int, default=13, help="cepstral coefficients 1..n (at most 15)")
    ap.add_argument("--stop-threshold", type=float, default=0.5)
    ap.add_argument("--limit", type=int, default=0, help="only the first N utterances (0: all)")
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error("--batch must be at least 1")
    if not 1 <= a.n_coef <= 15:
        ap.error("--n-coef must be 1..15")
    return a


def evaluate_corpus(model, batches, out_dir, n_coef=13, stop_threshold=0.5):
    """Score every batch of (ids, text, text_len, mel, mel_len) with model.evaluate and write
    out_dir/eval.json; returns the manifest."""
    utts = {}
    num = den = 0.0
    failed = 0
    for ids, text, text_len, mel, mel_len in batches:
        max_len = min(2 * mel.shape[1], model.cfg.max_len - 1, DTW_MAX_FRAMES)
        r = model.evaluate(text, text_len, mel, mel_len, max_len=max_len, stop_threshold=stop_threshold,
                           n_coef=n_coef)
        mcd, plen = r.mcd.float().cpu().tolist(), r.length.cpu().tolist()
        hyp, ref = r.hyp_len.cpu().tolist(), r.ref_len.cpu().tolist()
        for i, uid in enumerate(ids):
            hit = int(hyp[i]) >= max_len
            bad = hit or int(hyp[i]) <= 0 or not math.isfinite(mcd[i])
            utts[uid] = {"mcd": None if not math.isfinite(mcd[i]) else mcd[i], "hyp_len": int(hyp[i]),
                         "ref_len": int(ref[i]), "path_length": int(plen[i]), "hit_max_len": bool(hit)}
            if bad:
                failed += 1
            else:
                num += mcd[i] * int(ref[i])
                den += int(ref[i])
    man = {"utterances": utts, "mean_mcd": num / den if den else None, "scored": len(utts) - failed,
           "failed": failed, "n_coef": n_coef, "max_len_factor": 2}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "eval.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    return man


def main(argv=None):
    a = parse_args(argv)
    from tt2.audio import MelExtractor
    from tt2.config import TTSConfig
    from tt2.data import LJSpeech, bucket_batches, collate
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

    def batches():   # one batch resident at a time
        for idx in index_batches:
            text, text_len, mel, mel_len = collate(ds, idx, mx)
            yield [ds.items[i][0] for i in idx], text, text_len.int(), mel, mel_len.int()

    man = evaluate_corpus(model, batches(), a.out, n_coef=a.n_coef, stop_threshold=a.stop_threshold)
    print(json.dumps({"out": a.out, "utterances": len(man["utterances"]), "mean_mcd": man["mean_mcd"],
                      "failed": man["failed"]}))


if __name__ == "__main__":
    main()
