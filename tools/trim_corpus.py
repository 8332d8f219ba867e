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
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _corpus_cli as cli  # noqa: E402


def parse_args(argv=None):
    return cli.parse_args(__doc__, "trimmed", argv, trim="")


def main(argv=None):
    a = parse_args(argv)
    from tt2.data import LJSpeech, trim_corpus

    man = trim_corpus(LJSpeech(a.src, sr=a.sr_in), a.out, cli.build_front(a), batch_size=a.batch)
    utts = man["utterances"].values()
    print(json.dumps({"out": a.out, "utterances": len(utts), "trimmer": man["trimmer"],
                      "samples_out": sum(u["samples_out"] for u in utts), "clipped": sum(u["clipped"] for u in utts),
                      "removed_seconds": round(man["removed_seconds"], 3), "empty": len(man["empty"])}))


if __name__ == "__main__":
    main()
