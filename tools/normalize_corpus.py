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
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _corpus_cli as cli  # noqa: E402


def parse_args(argv=None):
    def own(ap):
        ap.add_argument("--target", type=float, default=-23.0, help="integrated loudness to reach, LKFS")
        ap.add_argument("--peak-db", type=float, default=-1.0, help="sample-peak ceiling after the gain, dBFS")
        ap.add_argument("--trim", action="store_true", help="remove leading and trailing silence first")
    return cli.parse_args(__doc__, "normalised", argv, own, trim="--trim: ")


def main(argv=None):
    a = parse_args(argv)
    from tt2.audio import LoudnessNormalizer
    from tt2.data import LJSpeech, normalize_corpus

    nz = LoudnessNormalizer(target=a.target, peak_db=a.peak_db, sr=cli.SR, resampler=cli.build_front(a, trim=a.trim))
    man = normalize_corpus(LJSpeech(a.src, sr=a.sr_in), a.out, nz, batch_size=a.batch)
    utts = man["utterances"].values()
    print(json.dumps({"out": a.out, "utterances": len(utts), "target": a.target, "peak_db": a.peak_db,
                      "stats": man["stats"], "unmeasured": len(man["unmeasured"]),
                      "clipped": sum(u["clipped"] for u in utts)}))


if __name__ == "__main__":
    main()
