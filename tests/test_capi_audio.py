"""CPU: the five entries of csrc/audio.hip are exported and bound, and every refusal
include/tt2_capi.h states for them returns TT2_E_INVALID before any launch, with the entry's own
name in the error text.  No compute calls (no GPU here); tests/test_gpu_audio_kernels.py shows on
the device that a refused call leaves its output untouched."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tt2_reflect_pad", "tt2_spec_magnitude", "tt2_spec_rephase", "tt2_overlap_add", "tt2_mel_rows")


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    bound = lib.load()
    for name in ENTRIES:
        assert hasattr(L, name) and name in lib.SIGNATURES and name in header, name
        assert getattr(bound, name).restype is ctypes.c_int


# Valid arguments of each entry (keyword -> value, in the C order) and the refusals the header
# states, each as the keywords it changes.  P stands for a host buffer: nothing is ever launched.
P = "buffer"
REFUSALS = {
    "tt2_reflect_pad": (
        dict(x=P, ldx=1300, lens=P, batch=2, len=1300, padded=P, padded_len=2560, pad=512),
        [dict(x=None), dict(padded=None), dict(batch=0), dict(batch=-1), dict(len=0), dict(len=-4),
         dict(pad=-1), dict(pad=-512), dict(pad=1300), dict(pad=2000, padded_len=8000),
         dict(padded_len=2323), dict(padded_len=0), dict(padded_len=-1),
         dict(ldx=1299), dict(ldx=0), dict(ldx=-1300),
         dict(pad=2 ** 30, len=2 ** 31 - 1, ldx=2 ** 31, padded_len=2 ** 31 + 100)]),     # len + 2 pad in 64 bits
    "tt2_spec_magnitude": (
        dict(spec=P, ld_spec=1032, m=10, n_bins=513, mag=P, ld_mag=516),
        [dict(spec=None), dict(mag=None), dict(m=0), dict(m=-3), dict(ld_spec=1025), dict(ld_spec=0),
         dict(ld_mag=512), dict(ld_mag=0), dict(ld_mag=-516)]),
    "tt2_spec_rephase": (
        dict(mag=P, ld_mag=516, est=P, ld_est=1032, m=10, n_bins=513, out=P, ld_out=1032),
        [dict(mag=None), dict(out=None), dict(m=0), dict(m=-1), dict(ld_mag=512), dict(ld_mag=0), dict(ld_mag=-1),
         dict(ld_out=1025), dict(ld_out=1540), dict(ld_out=0), dict(ld_est=1025), dict(ld_est=0),
         dict(est=None, ld_mag=512)]),
    "tt2_overlap_add": (
        dict(frames=P, ld_frames=1024, lens=P, batch=2, len=1280, rows_per_utt=9, n_fft=1024, hop=256, y=P,
             ld_y=1280),
        [dict(frames=None), dict(y=None), dict(batch=0), dict(batch=-2), dict(len=0), dict(len=-1), dict(hop=0),
         dict(hop=-256), dict(n_fft=255), dict(n_fft=0), dict(ld_frames=1023), dict(ld_frames=0),
         dict(rows_per_utt=8), dict(rows_per_utt=0), dict(rows_per_utt=-9), dict(ld_y=1279), dict(ld_y=0),
         dict(ld_y=-1280)]),
    "tt2_mel_rows": (
        dict(rows=P, ld_rows=80, mel=P, frames=P, batch=2, t=6, n_mels=80, rows_per_utt=9, clamp=1e-5, scatter=0),
        [dict(rows=None), dict(mel=None), dict(batch=0), dict(batch=-1), dict(t=0), dict(t=-1), dict(t=10),
         dict(n_mels=0), dict(n_mels=-80), dict(ld_rows=79), dict(ld_rows=0), dict(clamp=0.0), dict(clamp=-1e-5),
         dict(clamp=float("nan")), dict(scatter=1, n_mels=0), dict(scatter=1, t=10), dict(scatter=1, ld_rows=79)]),
}


def call(L, name, args, buf):
    vals = [ctypes.addressof(buf) if v == P else v for v in args.values()]
    return getattr(L, name)(*vals, None)


def test_every_stated_refusal(lib):
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    E = lib.E_INVALID
    assert E == -1
    for name, (valid, refused) in REFUSALS.items():
        assert len(valid) + 1 == len(lib.SIGNATURES[name][0]), name          # + the stream
        for kw in refused:
            assert set(kw) <= set(valid), (name, kw)
            # something else first, so that the message read afterwards belongs to this call
            assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()
            assert call(L, name, dict(valid, **kw), buf) == E, (name, kw)
            assert name.encode() in L.tt2_last_error(), (name, kw, L.tt2_last_error())


def test_header_states_the_refusals_and_ragged_rules(lib):
    """The sentences the tests pin are in the header's comments of these entries."""
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    sec = header[header.index("audio data path"):]
    sec = " ".join(sec.replace("*", " ").split())
    for phrase in ("pad < 0 or pad >= len", "ldx < len when batch > 1", "ld_y < len when batch > 1",
                   "ld_mag < n_bins", "n_mels <= 0", "an entry above len counts as len",
                   "len_b <= 0 gives a row of zeros", "0 < len_b <= pad", "clamped into [0, len_b)",
                   "an entry above t counts as t", "frames[b] <= 0"):
        assert phrase in sec, phrase
    assert sec.count("Refused:") >= 5
