"""What resample_corpus.py, trim_corpus.py and normalize_corpus.py share: the package on sys.path, the
--in / --out / --sr-in / --batch and trimmer options, and the chain in front of a tool's own stage."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "transformer-tacotron2_amd"))
SR = 22050


def parse_args(doc, what, argv, own=lambda ap: None, trim=None, sr_in=SR):
    """The tool's arguments: --in, --out (of the `what` corpus), --sr-in (sr_in=None: required), the
    options that own(ap) adds, the trimmer's (trim: the prefix of their help; None: none), --batch."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in", dest="src", required=True, help="corpus root (metadata.csv, wavs/) at --sr-in")
    ap.add_argument("--out", required=True, help=f"root of the {what} corpus")
    ap.add_argument("--sr-in", type=int, default=sr_in, required=sr_in is None, help="sample rate of the corpus' files"
                    + ("" if sr_in is None else " (other than 22050: resampled first)"))
    own(ap)
    if trim is not None:
        ap.add_argument("--top-db", type=float, default=60.0, help=trim + "frames this far below the loudest one are silence")
        ap.add_argument("--frame", type=int, default=2048, help=trim + "frame length in samples at 22.05 kHz"
                        + ("" if trim else ": 2 * r * hop"))
        ap.add_argument("--hop", type=int, default=512, help=trim + "frame hop in samples at 22.05 kHz")
        ap.add_argument("--keep", type=int, default=0, help=trim + "samples kept either side of the loud stretch")
    ap.add_argument("--batch", type=int, default=16)
    return ap.parse_args(argv)


def build_front(a, trim=True):
    """A Resampler to 22.05 kHz when --sr-in is another rate, behind a SilenceTrimmer when `trim`; or None."""
    from tt2.audio import Resampler, SilenceTrimmer
    front = Resampler(a.sr_in, SR) if a.sr_in != SR else None
    if trim:
        front = SilenceTrimmer(top_db=a.top_db, frame=a.frame, hop=a.hop, keep=a.keep, sr=SR, resampler=front)
    return front
