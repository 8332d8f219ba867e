"""An LJSpeech-format corpus with leading and trailing silence removed (GPU).

A thin command line over tt2.data.trim_corpus: every wavs/<id>.wav of --in (PCM16 / PCM32 / float,
all at --sr-in) goes through tt2.audio.SilenceTrimmer, the frame-energy rule of tt2_trim
(include/tt2_capi.h has the definition; with --keep 0 it is librosa.effects.trim's with ref = np.max),
and is written as PCM16 mono at 22.05 kHz under --out/wavs.  When --sr-in is not 22050 the batch is
resampled first (tt2.audio.Resampler's default bank), in the same pass.  metadata.csv is copied
without the lines of utterances that were trimmed to nothing, which are not written either;
--out/trim.json records the parameters and per utterance the samples in, the first kept sample, the
samples out and how many samples the PCM16 range clipped, the seconds removed in total and the ids
of the empty utterances.  --out is then a corpus every other tool here reads as it is.

The defaults are librosa's; they were chosen without a speech corpus at hand.

    python tools/trim_corpus.py --in /data/VCTK-lj --out /data/VCTK-22k-trim --sr-in 48000 \
        [--top-db 60] [--frame 2048] [--hop 512] [--keep 0] [--batch 16]
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
    ap.add_argument("--out", required=True, help="root of the trimmed corpus")
    ap.add_argument("--sr-in", type=int, default=SR, help="sample rate of the corpus' files (other than 22050: resampled first)")
    ap.add_argument("--top-db", type=float, default=60.0, help="frames this far below the loudest one are silence")
    ap.add_argument("--frame", type=int, default=2048, help="frame length in samples at 22.05 kHz: 2 * r * hop")
    ap.add_argument("--hop", type=int, default=512, help="frame hop in samples at 22.05 kHz")
    ap.add_argument("--keep", type=int, default=0, help="samples kept either side of the loud stretch")
    ap.add_argument("--batch", type=int, default=16)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    from tt2.audio import Resampler, SilenceTrimmer
    from tt2.data import LJSpeech, trim_corpus

    ds = LJSpeech(a.src, sr=a.sr_in)
    rs = Resampler(a.sr_in, SR) if a.sr_in != SR else None
    tr = SilenceTrimmer(top_db=a.top_db, frame=a.frame, hop=a.hop, keep=a.keep, sr=SR, resampler=rs)
    man = trim_corpus(ds, a.out, tr, batch_size=a.batch)
    utts = man["utterances"].values()
    print(json.dumps({"out": a.out, "utterances": len(utts), "trimmer": man["trimmer"],
                      "samples_out": sum(u["samples_out"] for u in utts), "clipped": sum(u["clipped"] for u in utts),
                      "removed_seconds": round(man["removed_seconds"], 3), "empty": len(man["empty"])}))


if __name__ == "__main__":
    main()
