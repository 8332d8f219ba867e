"""An LJSpeech-format corpus brought to one loudness (GPU).

A thin command line over tt2.data.normalize_corpus: every wavs/<id>.wav of --in (PCM16 / PCM32 /
float, all at --sr-in) goes through tt2.audio.LoudnessNormalizer, the integrated loudness of ITU-R
BS.1770-4 (K-weighting, 400 ms blocks every 100 ms, the -70 LKFS and -10 LU gates; include/tt2_capi.h
has the definition of tt2_loudness), gets one gain that brings it to --target LKFS unless its sample
peak would then pass --peak-db dBFS (then the peak sets the gain), and is written as PCM16 mono at
22.05 kHz under --out/wavs.  When --sr-in is not 22050 the batch is resampled first
(tt2.audio.Resampler's default bank), and with --trim leading and trailing silence goes first as well
(tt2.audio.SilenceTrimmer, --top-db / --frame / --hop / --keep as in tools/trim_corpus.py), all in the
same pass.  metadata.csv is copied; --out/loudness.json records the parameters, per utterance the
loudness before, the gain in dB, the sample peak before, whether the peak limited the gain and how
many samples the PCM16 range clipped, the ids of the unmeasured utterances (no 400 ms block above
the gates: copied at gain 1), and the corpus' mean, lowest and highest loudness before.  --out is
then a corpus every other tool here reads as it is.  No limiter, no true-peak measurement.

The defaults (-23 LUFS, -1 dBFS) are EBU R128's; they were chosen without a speech corpus at hand.

    python tools/normalize_corpus.py --in /data/VCTK-lj --out /data/VCTK-22k-norm --sr-in 48000 \
        [--target -23] [--peak-db -1] [--trim [--top-db 60] [--frame 2048] [--hop 512] [--keep 0]] [--batch 16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-tacotron2_amd"))

SR = 22050


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in", dest="src", required=True, help="corpus root (metadata.csv, wavs/) at --sr-in")
    ap.add_argument("--out", required=True, help="root of the normalised corpus")
    ap.add_argument("--sr-in", type=int, default=SR, help="sample rate of the corpus' files (other than 22050: resampled first)")
    ap.add_argument("--target", type=float, default=-23.0, help="integrated loudness to reach, LKFS")
    ap.add_argument("--peak-db", type=float, default=-1.0, help="sample-peak ceiling after the gain, dBFS")
    ap.add_argument("--trim", action="store_true", help="remove leading and trailing silence first")
    ap.add_argument("--top-db", type=float, default=60.0, help="--trim: frames this far below the loudest one are silence")
    ap.add_argument("--frame", type=int, default=2048, help="--trim: frame length in samples at 22.05 kHz")
    ap.add_argument("--hop", type=int, default=512, help="--trim: frame hop in samples at 22.05 kHz")
    ap.add_argument("--keep", type=int, default=0, help="--trim: samples kept either side of the loud stretch")
    ap.add_argument("--batch", type=int, default=16)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    from tt2.audio import LoudnessNormalizer, Resampler, SilenceTrimmer
    from tt2.data import LJSpeech, normalize_corpus

    ds = LJSpeech(a.src, sr=a.sr_in)
    front = Resampler(a.sr_in, SR) if a.sr_in != SR else None
    if a.trim:
        front = SilenceTrimmer(top_db=a.top_db, frame=a.frame, hop=a.hop, keep=a.keep, sr=SR, resampler=front)
    nz = LoudnessNormalizer(target=a.target, peak_db=a.peak_db, sr=SR, resampler=front)
    man = normalize_corpus(ds, a.out, nz, batch_size=a.batch)
    utts = man["utterances"].values()
    print(json.dumps({"out": a.out, "utterances": len(utts), "target": a.target, "peak_db": a.peak_db,
                      "stats": man["stats"], "unmeasured": len(man["unmeasured"]),
                      "clipped": sum(u["clipped"] for u in utts)}))


if __name__ == "__main__":
    main()
