"""CPU: tt2_yin is exported and bound, the ctypes struct of tt2_yin_args matches the C layout
(test_capi_dtw.py's approach), every host-side refusal behaves as the header states, the
zero-size calls succeed, and the Python surface is as documented.  No compute calls (no GPU here)."""
import ctypes
import inspect
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_yin_symbol_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "tt2_yin")
    assert "tt2_yin" in lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    for name in ("tt2_yin", "tt2_yin_args", "TT2_YIN_FRAME", "TT2_YIN_WINDOW", "TT2_YIN_MAX_LAG"):
        assert name in header, name
    bound = lib.load()
    assert bound.tt2_yin.argtypes[0]._type_ is lib.YinArgs
    assert bound.tt2_yin.restype is ctypes.c_int
    assert (lib.YIN_FRAME, lib.YIN_WINDOW, lib.YIN_MAX_LAG) == (1024, 512, 511)


def test_python_surface(lib):
    from tt2 import audio, data, evaluate, ops
    assert audio.Pitch._fields == ("f0", "voiced", "aperiodicity", "energy", "frames")
    assert evaluate.F0Score._fields == ("rmse_cents", "vuv_error", "gpe", "voiced_pairs")
    assert list(inspect.signature(ops.yin).parameters) == ["x", "utt_stride", "f0", "lag", "aper", "energy", "hop",
                                                           "tau_min", "tau_max", "sr", "threshold", "frames", "cmnd"]
    sig = inspect.signature(audio.PitchExtractor.__init__).parameters
    assert list(sig) == ["self", "extractor", "fmin", "fmax", "threshold"]
    assert (sig["extractor"].default, sig["fmin"].default, sig["fmax"].default, sig["threshold"].default) == \
        (None, 65.0, 600.0, 0.1)
    assert list(inspect.signature(audio.PitchExtractor.__call__).parameters) == ["self", "audio", "lens"]
    assert list(inspect.signature(audio.phoneme_average).parameters) == ["values", "durations", "mask"]
    assert list(inspect.signature(evaluate.f0_metrics).parameters) == ["f0_hyp", "f0_ref", "path_hyp", "path_ref",
                                                                      "length"]
    sig = inspect.signature(evaluate.f0_dtw).parameters
    assert list(sig) == ["wav_hyp", "hyp_len", "wav_ref", "ref_len", "n_coef", "pitch"]
    assert sig["n_coef"].default == 13 and sig["pitch"].default is None
    sig = inspect.signature(data.extract_pitch).parameters
    assert list(sig) == ["batches", "out_dir", "extractor", "durations_dir"] and sig["durations_dir"].default is None


def test_lag_range_of_the_extractor(lib):
    """tau_min = ceil(sr / fmax), tau_max = min(511, floor(sr / fmin)); no device work at construction."""
    from tt2 import audio

    class NoMel:   # the extractor only keeps it
        dev = "cpu"

    p = audio.PitchExtractor(NoMel())
    assert (p.tau_min, p.tau_max) == (math.ceil(22050 / 600.0), math.floor(22050 / 65.0)) == (37, 339)
    p = audio.PitchExtractor(NoMel(), fmin=30.0, fmax=22050.0)
    assert (p.tau_min, p.tau_max) == (1, 511)
    assert audio.PitchExtractor(NoMel(), fmin=441.0, fmax=441.0).tau_min == 50
    assert p.params()["tau_max"] == 511 and p.params()["hop"] == 256 and p.params()["threshold"] == 0.1
    with pytest.raises(ValueError):
        audio.PitchExtractor(NoMel(), fmin=700.0, fmax=600.0)
    with pytest.raises(ValueError):
        audio.PitchExtractor(NoMel(), threshold=0.0)
    with pytest.raises(ValueError):
        audio.PitchExtractor(NoMel(), fmin=20.0, fmax=40.0)   # every lag beyond 511


def test_host_refusals_and_zero_sizes(lib):
    """Requests refused with TT2_E_INVALID before any launch (there is no GPU here: a launch would
    fail otherwise than with E_INVALID), and the zero-size calls return TT2_OK without one."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    a = lib.YinArgs()
    a.x = a.f0 = a.lag = a.aper = a.energy = p
    a.utt_stride, a.cmnd_ld = 4096, 0
    a.batch, a.t, a.hop, a.tau_min, a.tau_max = 2, 3, 256, 36, 340
    a.sr, a.threshold = 22050.0, 0.1

    def rc(**kw):
        b = lib.YinArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        return L.tt2_yin(ctypes.byref(b), None)

    E = lib.E_INVALID
    assert E == -1
    refused = [dict(tau_min=0), dict(tau_min=-3), dict(tau_min=341), dict(tau_max=512), dict(tau_min=500, tau_max=499),
               dict(hop=0), dict(hop=-256), dict(utt_stride=-1), dict(batch=-1), dict(t=-1),
               dict(sr=0.0), dict(sr=-1.0), dict(sr=float("inf")), dict(sr=float("nan")),
               dict(threshold=0.0), dict(threshold=-0.1), dict(threshold=float("inf")), dict(threshold=float("nan")),
               dict(f0=None), dict(lag=None), dict(aper=None), dict(energy=None), dict(x=None),
               dict(cmnd=p, cmnd_ld=340), dict(cmnd=p, cmnd_ld=0), dict(cmnd=p, cmnd_ld=-1)]
    for kw in refused:
        # something else first, so that the message read afterwards belongs to this call
        assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()
        assert rc(**kw) == E, kw
        assert b"tt2_yin" in L.tt2_last_error(), kw
    assert L.tt2_yin(None, None) == E
    # nothing to do: success without a launch, also with a null x, and still refused when malformed
    assert rc(batch=0) == 0 and rc(t=0) == 0 and rc(batch=0, t=0, x=None) == 0 and rc(t=0, x=None) == 0
    assert rc(batch=0, cmnd=p, cmnd_ld=341) == 0
    assert rc(batch=0, tau_min=0) == E and rc(t=0, f0=None) == E and rc(t=0, cmnd=p, cmnd_ld=340) == E


def test_yin_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and the struct's size, from a tiny host program."""
    structs = {"tt2_yin_args": lib.YinArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("frame value %d\\n", TT2_YIN_FRAME);\n'
    prog += 'printf("window value %d\\n", TT2_YIN_WINDOW);\n'
    prog += 'printf("max_lag value %d\\n", TT2_YIN_MAX_LAG);\n'
    prog += "return 0;}\n"
    # skipped only where the program cannot be built at all; a compile error is a failure
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc or no hip_runtime_api.h on this machine")
    src, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(src, "w").write(prog)
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    consts = {"frame": lib.YIN_FRAME, "window": lib.YIN_WINDOW, "max_lag": lib.YIN_MAX_LAG}
    seen = 0
    for line in filter(None, subprocess.run([exe], capture_output=True, text=True).stdout.split("\n")):
        name, field, val = line.split()
        if name in consts:
            assert int(val) == consts[name]
        elif field == "size":
            assert ctypes.sizeof(structs[name]) == int(val), name
        else:
            assert getattr(structs[name], field).offset == int(val), (name, field)
        seen += 1
    assert seen == 3 + sum(1 + len(c._fields_) for c in structs.values())
