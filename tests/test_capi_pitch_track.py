"""CPU: tt2_pitch_track is exported and bound, the ctypes struct of tt2_pitch_track_args matches the
C layout (test_capi_yin.py's approach), every host-side refusal behaves as the header states, the
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


def test_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "tt2_pitch_track") and hasattr(L, "tt2_pitch_track_workspace_size")
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    for name in ("tt2_pitch_track", "tt2_pitch_track_args", "tt2_pitch_track_workspace_size",
                 "TT2_PITCH_TRACK_MAX_FRAMES"):
        assert name in header, name
    bound = lib.load()
    assert bound.tt2_pitch_track.argtypes[0]._type_ is lib.PitchTrackArgs
    assert bound.tt2_pitch_track.restype is ctypes.c_int
    assert bound.tt2_pitch_track_workspace_size.restype is ctypes.c_size_t
    assert lib.PITCH_TRACK_MAX_FRAMES == 4096


def test_workspace_size(lib):
    ws = lib.load().tt2_pitch_track_workspace_size
    assert ws(0, 800, 37, 339) == 0 and ws(16, 0, 37, 339) == 0 and ws(0, 0, 37, 339) == 0
    assert ws(16, 800, 37, 339) == 16 * 800 * (303 + 1) * 4      # V of the 303 lags and U, f32
    assert ws(1, 1, 40, 40) == 8 and ws(2, 4096, 1, 511) == 2 * 4096 * 512 * 4
    assert ws(64, 4096, 1, 511) == 64 * 4096 * 512 * 4            # past 2^31 - 1: size_t arithmetic


def test_python_surface(lib):
    from tt2 import audio, ops
    assert audio.PitchTrack._fields == ("pitch", "lag", "cost")
    assert list(inspect.signature(ops.pitch_track).parameters) == [
        "cmnd", "frames", "f0", "lag", "cost", "tau_min", "tau_max", "sr", "pos", "jump", "switch", "unvoiced", "ws"]
    sig = inspect.signature(audio.PitchTracker.__init__).parameters
    assert list(sig) == ["self", "extractor", "jump", "switch", "unvoiced"]
    assert (sig["extractor"].default, sig["jump"].default, sig["switch"].default, sig["unvoiced"].default) == \
        (None, 1.0, 0.1, 0.2)
    assert list(inspect.signature(audio.PitchTracker.__call__).parameters) == ["self", "audio", "lens"]
    assert list(inspect.signature(audio.PitchTracker.track).parameters) == ["self", "audio", "lens"]


def test_params_on_a_stub_extractor(lib):
    """params() is the extractor's dict plus the tracker's four keys; no device work at construction."""
    from tt2 import audio

    class NoMel:
        dev = "cpu"

    px = audio.PitchExtractor(NoMel())
    tr = audio.PitchTracker(px)
    assert tr.mx is px.mx and (tr.tau_min, tr.tau_max) == (37, 339)
    assert tr.params() == {**px.params(), "track": "viterbi", "jump": 1.0, "switch": 0.1, "unvoiced": 0.2}
    assert audio.PitchTracker(px, jump=0.5, switch=0.0, unvoiced=2).params()["jump"] == 0.5
    pos = tr.pos()
    assert pos.dtype.is_floating_point and pos.shape == (340,) and pos[0] == 0 and pos[256] == 8.0 and pos[1] == 0
    for kw in (dict(jump=-1.0), dict(switch=float("nan")), dict(unvoiced=float("inf"))):
        with pytest.raises(ValueError):
            audio.PitchTracker(px, **kw)


def test_host_refusals_and_zero_sizes(lib):
    """Requests refused with TT2_E_INVALID before any launch (there is no GPU here: a launch would
    fail otherwise than with E_INVALID), and the calls with nothing to do return TT2_OK."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    a = lib.PitchTrackArgs()
    a.cmnd = a.frames = a.pos = a.f0 = a.lag = a.cost = a.workspace = p
    a.workspace_bytes = 2 * 3 * 306 * 4
    a.cmnd_ld = 341
    a.batch, a.t, a.tau_min, a.tau_max = 2, 3, 36, 340
    a.sr, a.jump, a.switch_cost, a.unvoiced = 22050.0, 1.0, 0.1, 0.2
    assert L.tt2_pitch_track_workspace_size(2, 3, 36, 340) == a.workspace_bytes

    def rc(**kw):
        b = lib.PitchTrackArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        return L.tt2_pitch_track(ctypes.byref(b), None)

    E = lib.E_INVALID
    assert E == -1
    inf, nan = float("inf"), float("nan")
    refused = [dict(tau_min=0), dict(tau_min=-3), dict(tau_min=341), dict(tau_max=512), dict(tau_min=500, tau_max=499),
               dict(batch=-1), dict(t=-1), dict(t=4097, workspace_bytes=1 << 40),
               dict(cmnd_ld=340), dict(cmnd_ld=0), dict(cmnd_ld=-1),
               dict(sr=0.0), dict(sr=-1.0), dict(sr=inf), dict(sr=nan),
               dict(jump=-0.5), dict(jump=inf), dict(jump=nan),
               dict(switch_cost=-0.5), dict(switch_cost=inf), dict(switch_cost=nan),
               dict(unvoiced=-0.5), dict(unvoiced=inf), dict(unvoiced=nan),
               dict(f0=None), dict(lag=None), dict(cost=None), dict(pos=None), dict(cmnd=None),
               dict(workspace=None), dict(workspace_bytes=a.workspace_bytes - 1), dict(workspace_bytes=0),
               dict(workspace=p + 2)]
    for kw in refused:
        # something else first, so that the message read afterwards belongs to this call
        assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()
        assert rc(**kw) == E, kw
        assert b"tt2_pitch_track" in L.tt2_last_error(), kw
    assert L.tt2_pitch_track(None, None) == E
    # nothing to do: success without a launch, also with a null cmnd and workspace; still refused when malformed
    assert rc(batch=0) == 0 and rc(batch=0, t=0) == 0
    assert rc(batch=0, cmnd=None, workspace=None, workspace_bytes=0, frames=None) == 0
    assert rc(batch=0, tau_min=0) == E and rc(t=0, f0=None) == E and rc(t=0, cmnd_ld=340) == E
    assert rc(batch=0, jump=-1.0) == E and rc(t=0, pos=None) == E
    # t = 0 with a batch is well-formed without cmnd or workspace: never E_INVALID (its memset of cost
    # needs a device, so it cannot succeed here; tests/test_gpu_pitch_track_kernels.py has the success)
    assert rc(t=0, cmnd=None, workspace=None, workspace_bytes=0) != E


def test_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and the struct's size, from a tiny host program."""
    structs = {"tt2_pitch_track_args": lib.PitchTrackArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_frames value %d\\n", TT2_PITCH_TRACK_MAX_FRAMES);\n'
    prog += "return 0;}\n"
    # skipped only where the program cannot be built at all; a compile error is a failure
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc or no hip_runtime_api.h on this machine")
    src, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(src, "w").write(prog)
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    consts = {"max_frames": lib.PITCH_TRACK_MAX_FRAMES}
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
