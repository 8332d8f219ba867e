"""CPU: tt2_loudness and its size query are exported and bound, the ctypes struct of tt2_loudness_args
matches the C layout (test_capi_trim.py's approach), the workspace size is what the source says, every
host-side refusal and the batch = 0 success behave as the header states, and the Python surface is as
documented.  No compute calls (no GPU here)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_loudness_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "tt2_loudness") and hasattr(L, "tt2_loudness_workspace_size")
    assert "tt2_loudness" in lib.SIGNATURES and "tt2_loudness_workspace_size" in lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    for name in ("tt2_loudness", "tt2_loudness_args", "tt2_loudness_workspace_size"):
        assert name in header, name
    bound = lib.load()
    assert bound.tt2_loudness.argtypes[0]._type_ is lib.LoudnessArgs
    assert bound.tt2_loudness.restype is ctypes.c_int
    assert bound.tt2_loudness_workspace_size.restype is ctypes.c_size_t


def test_workspace_size(lib):
    """Gains, then per segment of 1024 samples a peak, a state of four doubles and min(1024, 1023 / step
    + 2) pieces, then n_in / step sub-block sums; every part padded to 16 bytes."""
    L = lib.load()

    def up(n):
        return (n + 15) // 16 * 16

    def want(B, n, step):
        nseg = -(-n // 1024)
        npiece = min(1024, 1023 // step + 2)
        return up(4 * B) + up(4 * B * nseg) + 32 * B * nseg + up(8 * B * nseg * npiece) + up(8 * B * (n // step))

    for B, n, step in [(1, 1, 1), (16, 204544, 2205), (3, 1000, 7), (5, 0, 4), (2, 2 ** 31 - 1, 1), (7, 4095, 4096),
                       (1, 1025, 1023), (3, 3000, 512)]:
        assert L.tt2_loudness_workspace_size(B, n, step) == want(B, n, step), (B, n, step)
    for B, n, step in [(0, 100, 4), (-1, 100, 4), (2, -1, 4), (2, 100, 0), (2, 100, -3)]:
        assert L.tt2_loudness_workspace_size(B, n, step) == 0


def test_python_surface(lib):
    from tt2 import audio, data, ops
    sig = inspect.signature(ops.loudness).parameters
    assert list(sig) == ["x", "step", "coef", "abs_sum", "rel_ratio", "target_ms", "ceiling", "lens", "y", "loud", "gain",
                         "peak", "limited", "energy", "workspace"]
    assert all(sig[k].default is None for k in list(sig)[7:])
    assert audio.Loudness._fields == ("loud", "peak", "energy")
    assert audio.Normalized._fields == ("audio", "lens", "loud", "gain", "peak", "limited")
    sig = inspect.signature(audio.LoudnessNormalizer.__init__).parameters
    assert list(sig) == ["self", "target", "peak_db", "sr", "resampler", "device"]
    assert [sig[k].default for k in list(sig)[1:]] == [-23.0, -1.0, 22050, None, "cuda"]
    for name in ("measure", "normalize", "__call__"):
        sig = inspect.signature(getattr(audio.LoudnessNormalizer, name)).parameters
        assert list(sig) == ["self", "audio", "lens"] and sig["lens"].default is None
    sig = inspect.signature(data.normalize_corpus).parameters
    assert list(sig) == ["ds", "out_root", "normalizer", "batch_size"] and sig["batch_size"].default == 16
    # the hooks a LoudnessNormalizer goes into are as they were
    assert list(inspect.signature(data.collate).parameters) == ["ds", "indices", "extractor", "device", "resampler"]
    assert list(inspect.signature(data.resample_corpus).parameters) == ["ds", "out_root", "resampler", "batch_size"]


def test_normalizer_construction_does_no_device_work(lib):
    from tt2 import audio
    n = audio.LoudnessNormalizer()
    assert (n.target, n.peak_db, n.sr, n.step, n.sr_in, n.sr_out, n.rel_ratio) == (-23.0, -1.0, 22050, 2205, 22050, 22050, 0.1)
    assert n.abs_sum == 4 * 2205 * 10.0 ** ((-70 + 0.691) / 10) and n.target_ms == 10.0 ** ((-23 + 0.691) / 10)
    assert n.ceiling == float(np.float32(10.0 ** (-1 / 20))) and n._ws.buf is None
    want = [1.479825350977746, -2.170728612856829, 0.860842484726552, -1.338305336066134, 0.508244558913602,
            1.0, -2.0, 1.0, -1.978397602590119, 0.978514419503251]
    assert len(n.coef) == 10 and max(abs(a - b) for a, b in zip(n.coef, want)) < 1e-12
    p = n.params()
    assert p["target"] == -23.0 and p["step"] == 2205 and p["coef"] == list(n.coef) and "resampler" not in p
    chain = audio.LoudnessNormalizer(resampler=audio.SilenceTrimmer(resampler=audio.Resampler(48000)))
    assert (chain.sr_in, chain.sr_out) == (48000, 22050)
    assert chain.params()["resampler"]["resampler"]["sr_in"] == 48000
    n = audio.LoudnessNormalizer(target=-16, peak_db=-3, sr=16000, resampler=audio.Resampler(48000, 16000))
    assert (n.step, n.sr_in, n.sr_out) == (1600, 48000, 16000)


def test_normalizer_refuses_bad_parameters(lib):
    from tt2 import audio
    for kw in (dict(sr=22055), dict(sr=0), dict(sr=-10), dict(sr=22050.5), dict(target=float("nan")),
               dict(target=float("inf")), dict(peak_db=float("nan"))):
        with pytest.raises(ValueError):
            audio.LoudnessNormalizer(**kw)
    with pytest.raises(ValueError, match="16000"):
        audio.LoudnessNormalizer(resampler=audio.Resampler(48000, 16000))
    with pytest.raises(ValueError):
        audio.kweighting(0)


def test_host_refusals_and_zero_sizes(lib):
    """Requests refused with TT2_E_INVALID before any launch (there is no GPU here: a launch would
    fail otherwise than with E_INVALID), and batch = 0 returns TT2_OK without one."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    a = lib.LoudnessArgs()
    a.x = a.lens = a.y = a.loud = a.gain = a.peak = a.limited = a.energy = a.workspace = p
    a.workspace_bytes = 2 ** 62
    a.x_ld, a.y_ld, a.energy_ld = 1000, 900, 11
    a.batch, a.n_in, a.n_out, a.step = 2, 1000, 900, 100
    a.coef = (ctypes.c_double * 10)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0)
    a.abs_sum, a.rel_ratio, a.target_ms, a.ceiling = 1.0, 0.1, 0.01, 0.9
    need = L.tt2_loudness_workspace_size(2, 1000, 100)

    def rc(**kw):
        b = lib.LoudnessArgs.from_buffer_copy(a)
        for k, v in kw.items():
            if k.startswith("coef"):
                b.coef[int(k[4:])] = v
            else:
                setattr(b, k, v)
        return L.tt2_loudness(ctypes.byref(b), None)

    E = lib.E_INVALID
    assert E == -1
    big = 2 ** 31 - 1
    nan, inf = float("nan"), float("inf")
    nothing = dict(y=None, loud=None, gain=None, peak=None, limited=None, energy=None)
    refused = [dict(step=0), dict(step=-1), dict(step=2 ** 29), dict(step=big, energy=None),
               dict(batch=-1), dict(n_in=-1), dict(n_out=-1),
               dict(x_ld=999), dict(x_ld=-1), dict(y_ld=899), dict(energy_ld=10), dict(energy_ld=0),
               dict(coef0=nan), dict(coef4=inf), dict(coef9=-inf), dict(coef5=nan),
               dict(abs_sum=-1e-300), dict(abs_sum=nan), dict(abs_sum=inf),
               dict(rel_ratio=-1e-9), dict(rel_ratio=1.0000001), dict(rel_ratio=nan),
               dict(target_ms=0.0), dict(target_ms=-1.0), dict(target_ms=nan), dict(target_ms=inf),
               dict(ceiling=0.0), dict(ceiling=-0.5), dict(ceiling=nan), dict(ceiling=inf),
               dict(x=None), nothing, dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace_bytes=0),
               # one work group per four segments of 1024 samples; 256 per utterance at most in the gain pass
               dict(batch=big, n_in=8192, x_ld=8192, y=None, energy=None),
               dict(batch=big, n_in=1, x_ld=1, n_out=big, y_ld=big, energy=None)]
    for kw in refused:
        # something else first, so that the message read afterwards belongs to this call
        assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()
        assert rc(**kw) == E, kw
        assert b"tt2_loudness" in L.tt2_last_error(), kw
    assert L.tt2_loudness(None, None) == E
    # the limits themselves are accepted as far as the host checks go (batch = 0: no launch)
    assert rc(batch=0, step=2 ** 29 - 1, energy=None) == 0 and rc(batch=0, rel_ratio=0.0) == 0
    assert rc(batch=0, rel_ratio=1.0) == 0 and rc(batch=0, abs_sum=0.0) == 0
    assert rc(batch=0, workspace_bytes=0, workspace=None) == 0 and rc(batch=0, x=None) == 0
    assert rc(batch=0, lens=None, y=None, loud=None, gain=None, peak=None, limited=None) == 0   # energy alone
    assert rc(batch=0, y=None, y_ld=0) == 0                       # y absent: its leading dimension is not looked at
    # and still refused when malformed
    assert rc(batch=0, step=0) == E and rc(batch=0, x_ld=999) == E and rc(batch=0, **nothing) == E
    assert rc(batch=0, coef3=nan) == E and rc(batch=0, ceiling=0.0) == E


def test_loudness_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and the struct's size, from a tiny host program."""
    structs = {"tt2_loudness_args": lib.LoudnessArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += "return 0;}\n"
    # skipped only where the program cannot be built at all; a compile error is a failure
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc or no hip_runtime_api.h on this machine")
    src, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(src, "w").write(prog)
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = 0
    for line in filter(None, subprocess.run([exe], capture_output=True, text=True).stdout.split("\n")):
        name, field, val = line.split()
        if field == "size":
            assert ctypes.sizeof(structs[name]) == int(val), name
        else:
            assert getattr(structs[name], field).offset == int(val), (name, field)
        seen += 1
    assert seen == sum(1 + len(c._fields_) for c in structs.values())
