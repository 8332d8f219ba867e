"""CPU: tt2_trim and its size query are exported and bound, the ctypes struct of tt2_trim_args matches
the C layout (test_capi_yin.py's approach), the workspace size is what the header says, every
host-side refusal and zero-size success behaves as the header states, and the Python surface is as
documented.  No compute calls (no GPU here)."""
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


def test_trim_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "tt2_trim") and hasattr(L, "tt2_trim_workspace_size")
    assert "tt2_trim" in lib.SIGNATURES and "tt2_trim_workspace_size" in lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    for name in ("tt2_trim", "tt2_trim_args", "tt2_trim_workspace_size", "TT2_TRIM_MAX_R"):
        assert name in header, name
    bound = lib.load()
    assert bound.tt2_trim.argtypes[0]._type_ is lib.TrimArgs
    assert bound.tt2_trim.restype is ctypes.c_int
    assert bound.tt2_trim_workspace_size.restype is ctypes.c_size_t
    assert lib.TRIM_MAX_R == 16


def test_workspace_size(lib):
    """(start, out) per utterance padded to 16 bytes, then ceil(n_in / hop) block sums per utterance."""
    L = lib.load()

    def want(B, n, hop):
        return ((8 * B + 15) // 16) * 16 + 4 * B * -(-n // hop)

    for B, n, hop in [(1, 1, 1), (16, 204544, 512), (3, 1000, 7), (5, 0, 4), (2, 2 ** 31 - 1, 1), (7, 4095, 4096)]:
        assert L.tt2_trim_workspace_size(B, n, hop) == want(B, n, hop), (B, n, hop)
    for B, n, hop in [(0, 100, 4), (-1, 100, 4), (2, -1, 4), (2, 100, 0), (2, 100, -3)]:
        assert L.tt2_trim_workspace_size(B, n, hop) == 0


def test_python_surface(lib):
    from tt2 import audio, data, ops
    sig = inspect.signature(ops.trim).parameters
    assert list(sig) == ["x", "y", "hop", "r", "keep", "ratio", "lens", "out_lens", "start", "energy", "workspace"]
    assert all(sig[k].default is None for k in ("lens", "out_lens", "start", "energy", "workspace"))
    assert audio.Trimmed._fields == ("audio", "lens", "start", "energy")
    sig = inspect.signature(audio.SilenceTrimmer.__init__).parameters
    assert list(sig) == ["self", "top_db", "frame", "hop", "keep", "sr", "resampler", "device"]
    assert [sig[k].default for k in list(sig)[1:]] == [60.0, 2048, 512, 0, 22050, None, "cuda"]
    sig = inspect.signature(audio.SilenceTrimmer.trim).parameters
    assert list(sig) == ["self", "audio", "lens", "want_energy"]
    assert sig["lens"].default is None and sig["want_energy"].default is False
    sig = inspect.signature(audio.SilenceTrimmer.__call__).parameters
    assert list(sig) == ["self", "audio", "lens"] and sig["lens"].default is None
    sig = inspect.signature(data.trim_corpus).parameters
    assert list(sig) == ["ds", "out_root", "trimmer", "batch_size"] and sig["batch_size"].default == 16
    # the hooks a SilenceTrimmer goes into are as they were
    assert list(inspect.signature(data.collate).parameters) == ["ds", "indices", "extractor", "device", "resampler"]
    assert list(inspect.signature(data.resample_corpus).parameters) == ["ds", "out_root", "resampler", "batch_size"]


def test_trimmer_construction_does_no_device_work(lib):
    import numpy as np
    from tt2 import audio
    t = audio.SilenceTrimmer()
    assert (t.top_db, t.frame, t.hop, t.r, t.keep, t.sr, t.sr_in, t.sr_out) == (60.0, 2048, 512, 2, 0, 22050, 22050, 22050)
    assert t.ratio == float(np.float32(1e-6)) and t._ws.buf is None
    assert t.params() == {"top_db": 60.0, "frame": 2048, "hop": 512, "r": 2, "keep": 0, "ratio": float(np.float32(1e-6)),
                          "sr": 22050}
    t = audio.SilenceTrimmer(top_db=30, frame=512, hop=256, keep=100)
    assert (t.r, t.keep) == (1, 100) and t.ratio == float(np.float32(10.0 ** -3.0))
    assert audio.SilenceTrimmer(frame=32 * 64, hop=64).r == 16
    rs = audio.Resampler(48000)
    t = audio.SilenceTrimmer(resampler=rs)
    assert (t.sr_in, t.sr_out) == (48000, 22050) and rs._taps is None
    assert t.params()["resampler"] == rs.params() and t.params()["top_db"] == 60.0
    t = audio.SilenceTrimmer(sr=16000, resampler=audio.Resampler(48000, 16000))
    assert (t.sr_in, t.sr_out) == (48000, 16000)


def test_trimmer_refuses_bad_parameters(lib):
    from tt2 import audio
    for kw in (dict(frame=2048, hop=512 * 3), dict(frame=1536, hop=512), dict(frame=512, hop=512), dict(frame=0, hop=512),
               dict(frame=34 * 64, hop=64), dict(frame=2048, hop=0), dict(frame=2048.5)):
        with pytest.raises(ValueError, match="TT2_TRIM_MAX_R"):
            audio.SilenceTrimmer(**kw)
    for kw in (dict(top_db=-1.0), dict(top_db=float("nan")), dict(top_db=float("inf")), dict(keep=-1), dict(keep=1.5)):
        with pytest.raises(ValueError):
            audio.SilenceTrimmer(**kw)
    with pytest.raises(ValueError, match="16000"):
        audio.SilenceTrimmer(resampler=audio.Resampler(48000, 16000))


def test_host_refusals_and_zero_sizes(lib):
    """Requests refused with TT2_E_INVALID before any launch (there is no GPU here: a launch would
    fail otherwise than with E_INVALID), and the zero-size calls return TT2_OK without one."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    a = lib.TrimArgs()
    a.x = a.lens = a.y = a.out_lens = a.start = a.energy = a.workspace = p
    a.workspace_bytes = 2 ** 62
    a.x_ld, a.y_ld, a.energy_ld = 1000, 900, 2
    a.batch, a.n_in, a.n_out, a.hop, a.r, a.keep, a.ratio = 2, 1000, 900, 512, 2, 0, 1e-6
    need = L.tt2_trim_workspace_size(2, 1000, 512)

    def rc(**kw):
        b = lib.TrimArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        return L.tt2_trim(ctypes.byref(b), None)

    E = lib.E_INVALID
    assert E == -1
    big = 2 ** 31 - 1
    refused = [dict(hop=0), dict(hop=-1), dict(r=0), dict(r=-1), dict(r=17),
               dict(hop=2 ** 26, r=16), dict(hop=2 ** 30, r=1), dict(hop=big, r=1),
               dict(keep=-1), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(ratio=-1e-9), dict(ratio=1.0000001),
               dict(batch=-1), dict(n_in=-1), dict(n_out=-1),
               dict(x_ld=999), dict(y_ld=899), dict(x_ld=-1), dict(energy_ld=1), dict(energy_ld=0),
               dict(y=None), dict(x=None), dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace_bytes=0),
               # 1024 work groups per utterance in the energy pass, 256 in the copy
               dict(batch=big, n_in=4096, x_ld=4096, hop=1, energy=None),
               dict(batch=big, n_in=1, x_ld=1, hop=1, n_out=big, y_ld=big, energy=None)]
    for kw in refused:
        # something else first, so that the message read afterwards belongs to this call
        assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()
        assert rc(**kw) == E, kw
        assert b"tt2_trim" in L.tt2_last_error(), kw
    assert L.tt2_trim(None, None) == E
    # the limits themselves are accepted as far as the host checks go (zero-size: no launch)
    assert rc(batch=0, r=16, hop=2 ** 26 - 1) == 0 and rc(batch=0, ratio=0.0) == 0 and rc(batch=0, ratio=1.0) == 0
    assert rc(batch=0, workspace_bytes=0, workspace=None) == 0 and rc(n_out=0, workspace_bytes=need) == 0
    # nothing to do: success without a launch, also with a null x, and still refused when malformed
    assert rc(batch=0) == 0 and rc(n_out=0) == 0 and rc(batch=0, x=None) == 0 and rc(n_out=0, x=None) == 0
    assert rc(batch=0, lens=None, out_lens=None, start=None, energy=None) == 0
    assert rc(n_out=0, n_in=0, x=None, x_ld=0) == 0
    assert rc(batch=0, hop=0) == E and rc(n_out=0, y=None) == E and rc(batch=0, r=17) == E
    assert rc(n_out=0, energy_ld=1) == E and rc(batch=0, x_ld=999) == E and rc(n_out=0, workspace_bytes=need - 1) == E


def test_trim_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and the struct's size, from a tiny host program."""
    structs = {"tt2_trim_args": lib.TrimArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_r value %d\\n", TT2_TRIM_MAX_R);\n'
    prog += "return 0;}\n"
    # skipped only where the program cannot be built at all; a compile error is a failure
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc or no hip_runtime_api.h on this machine")
    src, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(src, "w").write(prog)
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    consts = {"max_r": lib.TRIM_MAX_R}
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
    assert seen == 1 + sum(1 + len(c._fields_) for c in structs.values())
