"""CPU: tt2_resample is exported and bound, the ctypes struct of tt2_resample_args matches the C
layout (test_capi_yin.py's approach), every host-side refusal behaves as the header states, the
zero-size calls succeed, and the Python surface is as documented.  No compute calls (no GPU here)."""
import ctypes
import inspect
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


def test_resample_symbol_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "tt2_resample")
    assert "tt2_resample" in lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    for name in ("tt2_resample", "tt2_resample_args", "TT2_RESAMPLE_MAX_TAPS", "TT2_RESAMPLE_MAX_PHASES"):
        assert name in header, name
    bound = lib.load()
    assert bound.tt2_resample.argtypes[0]._type_ is lib.ResampleArgs
    assert bound.tt2_resample.restype is ctypes.c_int
    assert (lib.RESAMPLE_MAX_TAPS, lib.RESAMPLE_MAX_PHASES) == (256, 1024)


def test_python_surface(lib):
    from tt2 import audio, data, ops
    assert list(inspect.signature(ops.resample).parameters) == ["x", "y", "bank", "up", "down", "half", "lens",
                                                                "out_lens"]
    sig = inspect.signature(ops.resample).parameters
    assert sig["lens"].default is None and sig["out_lens"].default is None
    assert audio.ResampleBank._fields == ("up", "down", "half", "taps")
    sig = inspect.signature(audio.resample_bank).parameters
    assert list(sig) == ["sr_in", "sr_out", "zeros", "rolloff", "beta"]
    assert (sig["zeros"].default, sig["rolloff"].default, sig["beta"].default) == (24, 0.9, 10.0)
    sig = inspect.signature(audio.Resampler.__init__).parameters
    assert list(sig) == ["self", "sr_in", "sr_out", "device", "zeros", "rolloff", "beta"]
    assert (sig["sr_out"].default, sig["device"].default, sig["zeros"].default, sig["rolloff"].default,
            sig["beta"].default) == (22050, "cuda", 24, 0.9, 10.0)
    assert list(inspect.signature(audio.Resampler.__call__).parameters) == ["self", "audio", "lens"]
    assert inspect.signature(audio.Resampler.__call__).parameters["lens"].default is None
    sig = inspect.signature(data.collate).parameters
    assert list(sig) == ["ds", "indices", "extractor", "device", "resampler"] and sig["resampler"].default is None
    sig = inspect.signature(data.LJSpeech.__init__).parameters
    assert list(sig) == ["self", "root", "use_normalized", "sr"] and sig["sr"].default == 22050
    sig = inspect.signature(data.resample_corpus).parameters
    assert list(sig) == ["ds", "out_root", "resampler", "batch_size"] and sig["batch_size"].default == 16
    assert list(inspect.signature(data.read_wav).parameters) == ["path"]


def test_resampler_construction_does_no_device_work(lib):
    """Rates, ratio and parameters of a Resampler; its bank stays on the host until the first call."""
    from tt2 import audio
    r = audio.Resampler(48000)
    assert (r.sr_in, r.sr_out, r.up, r.down, r.half) == (48000, 22050, 147, 320, 59) and r._taps is None
    assert r.params() == {"sr_in": 48000, "sr_out": 22050, "up": 147, "down": 320, "half": 59, "zeros": 24,
                          "rolloff": 0.9, "beta": 10.0}
    assert [r.out_len(n) for n in (0, 1, 320, 321, 48000)] == [0, 1, 147, 148, 22050]
    r = audio.Resampler(44100, zeros=16, rolloff=0.95, beta=8.0)
    assert (r.up, r.down) == (1, 2) and r.params()["zeros"] == 16 and r.params()["beta"] == 8.0
    with pytest.raises(ValueError):
        audio.Resampler(48000, rolloff=1.5)
    with pytest.raises(ValueError, match="TT2_RESAMPLE_MAX_TAPS"):
        audio.Resampler(192000)


def test_identity_resampler_returns_its_inputs(lib):
    """sr_in == sr_out: no launch (this machine has no GPU to launch on), the inputs come back."""
    import torch
    from tt2 import audio
    r = audio.Resampler(22050)
    x = torch.randn(2, 100)
    lens = torch.tensor([100, 40], dtype=torch.int32)
    y, n = r(x, lens)
    assert y is x and n is lens
    y, n = r(x)
    assert y is x and n.dtype == torch.int32 and n.tolist() == [100, 100]


def test_host_refusals_and_zero_sizes(lib):
    """Requests refused with TT2_E_INVALID before any launch (there is no GPU here: a launch would
    fail otherwise than with E_INVALID), and the zero-size calls return TT2_OK without one."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    a = lib.ResampleArgs()
    a.x = a.bank = a.y = a.lens = a.out_lens = p
    a.x_ld, a.y_ld, a.bank_ld = 640, 300, 31
    a.batch, a.n_in, a.n_out, a.up, a.down, a.half = 2, 640, 294, 147, 320, 14

    def rc(**kw):
        b = lib.ResampleArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        return L.tt2_resample(ctypes.byref(b), None)

    E = lib.E_INVALID
    assert E == -1
    big = 2 ** 31 - 1
    refused = [dict(up=0), dict(up=-1), dict(down=0), dict(down=-5), dict(up=1025),
               dict(half=-1), dict(half=128, bank_ld=300), dict(half=2 ** 30, bank_ld=2 ** 40),
               dict(batch=-1), dict(n_in=-1), dict(n_out=-1),
               dict(x_ld=639), dict(y_ld=293), dict(bank_ld=28), dict(bank_ld=0), dict(x_ld=-1),
               dict(bank=None), dict(y=None), dict(x=None),
               # work groups: 64 residues x 4 period groups of 8 per group of (1024, 1023, 1)
               dict(batch=big, n_out=big, y_ld=big, up=1, down=1, half=0),
               dict(batch=big, n_out=big, y_ld=big, up=1024, down=1023, half=1)]
    for kw in refused:
        # something else first, so that the message read afterwards belongs to this call
        assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()
        assert rc(**kw) == E, kw
        assert b"tt2_resample" in L.tt2_last_error(), kw
    assert L.tt2_resample(None, None) == E
    # the largest filter and phase count are accepted as far as the host checks go (zero-size: no launch)
    assert rc(batch=0, half=127, bank_ld=255, up=1024) == 0
    # nothing to do: success without a launch, also with a null x, and still refused when malformed
    assert rc(batch=0) == 0 and rc(n_out=0) == 0 and rc(batch=0, x=None) == 0 and rc(n_out=0, x=None) == 0
    assert rc(batch=0, lens=None, out_lens=None) == 0 and rc(n_out=0, n_in=0, x=None, x_ld=0) == 0
    assert rc(batch=0, up=0) == E and rc(n_out=0, y=None) == E and rc(batch=0, bank=None) == E
    assert rc(n_out=0, half=128, bank_ld=300) == E and rc(batch=0, x_ld=639) == E


def test_resample_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and the struct's size, from a tiny host program."""
    structs = {"tt2_resample_args": lib.ResampleArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_taps value %d\\n", TT2_RESAMPLE_MAX_TAPS);\n'
    prog += 'printf("max_phases value %d\\n", TT2_RESAMPLE_MAX_PHASES);\n'
    prog += "return 0;}\n"
    # skipped only where the program cannot be built at all; a compile error is a failure
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc or no hip_runtime_api.h on this machine")
    src, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(src, "w").write(prog)
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    consts = {"max_taps": lib.RESAMPLE_MAX_TAPS, "max_phases": lib.RESAMPLE_MAX_PHASES}
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
    assert seen == 2 + sum(1 + len(c._fields_) for c in structs.values())
