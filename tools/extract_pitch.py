"""Frame-level pitch and energy of an LJSpeech-format corpus (GPU).

A thin command line over tt2.data.extract_pitch: YIN pitch and RMS energy on the mel frame grid
(tt2.audio.PitchExtractor, one tt2_yin launch per batch), <id>.f0.npy and <id>.energy.npy (f32
[frames]) per utterance and a pitch.json manifest with the corpus statistics in --out.  With
--durations pointing at the output of tools/extract_durations.py, also the phoneme averages
<id>.f0_ph.npy and <id>.energy_ph.npy: with the durations, the targets of a FastSpeech 2 style
student.

With --track viterbi the F0 and the voicing come from tt2.audio.PitchTracker instead: one path per
utterance through the lags and an unvoiced state over the same d' (one tt2_pitch_track launch
more per batch), which removes the octave-up frames and mid-vowel dropouts of the per-frame
decision.  --jump, --switch and --unvoiced are its three costs; pitch.json records them.

    python tools/extract_pitch.py --data /data/LJSpeech-1.1 --out pitch/ [--durations durations/] \
        [--batch 16] [--fmin 65] [--fmax 600] [--threshold 0.1] [--limit N] \
        [--track viterbi [--jump 1.0] [--switch 0.1] [--unvoiced 0.2]]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-tacotron2_amd"))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="LJSpeech root (metadata.csv, wavs/)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--durations", default=None, help="directory of <id>.npy durations (tools/extract_durations.py)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--fmin", type=float, default=65.0)
    ap.add_argument("--fmax", type=float, default=600.0)
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--limit", type=int, default=0, help="only the first N utterances (0: all)")
    ap.add_argument("--track", choices=["none", "viterbi"], default="none",
                    help="viterbi: F0 and voicing from tt2.audio.PitchTracker (default: the per-frame decision)")
    ap.add_argument("--jump", type=float, default=1.0, help="--track viterbi: cost of moving one octave")
    ap.add_argument("--switch", type=float, default=0.1, help="--track viterbi: cost of a change of voicing")
    ap.add_argument("--unvoiced", type=float, default=0.2, help="--track viterbi: cost of an unvoiced frame")
    return ap.parse_args(argv)


def make_extractor(a):
    """The extractor the arguments ask for: a PitchExtractor, inside a PitchTracker with --track viterbi."""
    from tt2 import audio

    px = audio.PitchExtractor(fmin=a.fmin, fmax=a.fmax, threshold=a.threshold)
    if a.track == "viterbi":
        px = audio.PitchTracker(px, jump=a.jump, switch=a.switch, unvoiced=a.unvoiced)
    return px


def main(argv=None):
    a = parse_args(argv)
    import torch

    from tt2.data import LJSpeech, extract_pitch

    ds = LJSpeech(a.data)
    px = make_extractor(a)
    n = min(len(ds), a.limit) if a.limit else len(ds)

    def batches():   # one batch resident at a time, in corpus order
        for i0 in range(0, n, a.batch):
            idx = range(i0, min(n, i0 + a.batch))
            wavs = [ds.wav(i) for i in idx]
            audio = torch.zeros(len(wavs), max(len(w) for w in wavs), dtype=torch.float32)
            for b, w in enumerate(wavs):
                audio[b, :len(w)] = torch.from_numpy(w)
            yield [ds.items[i][0] for i in idx], audio, torch.tensor([len(w) for w in wavs], dtype=torch.int32)

    man = extract_pitch(batches(), a.out, px, durations_dir=a.durations)
    print(json.dumps({"out": a.out, "utterances": len(man["utterances"]), "log_f0": man["log_f0"],
                      "energy": man["energy"]}))


if __name__ == "__main__":
    main()
