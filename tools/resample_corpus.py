"""An LJSpeech-format corpus at another sample rate, rewritten at 22.05 kHz (GPU).

A thin command line over tt2.data.resample_corpus: every wavs/<id>.wav of --in (PCM16 / PCM32 /
float, all at --sr-in) goes through tt2.audio.Resampler, the polyphase Kaiser-windowed sinc of
tt2_resample (include/tt2_capi.h has the definition), one launch per batch, and is written as PCM16
mono at --sr under --out/wavs; metadata.csv is copied, and --out/resample.json records the filter
(rates, up, down, half, zeros, rolloff, beta) and per utterance the samples in and out and how many
samples the PCM16 range clipped.  --out is then a corpus every other tool here reads as it is.

    python tools/resample_corpus.py --in /data/VCTK-lj --out /data/VCTK-22k --sr-in 48000 \
        [--sr 22050] [--zeros 24] [--rolloff 0.9] [--beta 10.0] [--batch 16]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _corpus_cli as cli  # noqa: E402


def parse_args(argv=None):
    def own(ap):
        ap.add_argument("--sr", type=int, default=22050, help="sample rate to write")
        ap.add_argument("--zeros", type=int, default=24, help="zero crossings of the sinc either side")
        ap.add_argument("--rolloff", type=float, default=0.9, help="cutoff as a fraction of the lower Nyquist")
        ap.add_argument("--beta", type=float, default=10.0, help="Kaiser window shape")
    return cli.parse_args(__doc__, "resampled", argv, own, sr_in=None)


def main(argv=None):
    a = parse_args(argv)
    from tt2.audio import Resampler
    from tt2.data import LJSpeech, resample_corpus

    rs = Resampler(a.sr_in, a.sr, zeros=a.zeros, rolloff=a.rolloff, beta=a.beta)
    man = resample_corpus(LJSpeech(a.src, sr=a.sr_in), a.out, rs, batch_size=a.batch)
    utts = man["utterances"].values()
    print(json.dumps({"out": a.out, "utterances": len(utts), "resampler": man["resampler"],
                      "samples_out": sum(u["samples_out"] for u in utts), "clipped": sum(u["clipped"] for u in utts)}))


if __name__ == "__main__":
    main()
