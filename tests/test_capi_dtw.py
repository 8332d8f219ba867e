"""CPU: the DTW entry points are exported and bound, the ctypes struct of tt2_dtw_args matches the C
layout (test_capi_mono.py's approach), the workspace query and every host-side refusal behave as
the header states, and the Python surface is as documented.  No compute calls (no GPU here)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tt2_dtw_workspace_size", "tt2_dtw")


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_dtw_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    for name in NEW + ("tt2_dtw_args", "TT2_DTW_MAX_FRAMES", "TT2_DTW_MAX_FEATS"):
        assert name in header, name
    bound = lib.load()
    assert bound.tt2_dtw.argtypes[0]._type_ is lib.DtwArgs
    assert bound.tt2_dtw_workspace_size.restype is ctypes.c_size_t
    assert (lib.DTW_MAX_FRAMES, lib.DTW_MAX_FEATS) == (2048, 32)


def test_python_surface(lib):
    from tt2 import evaluate, ops
    from tt2.model import Evaluation, TransformerTTS
    assert evaluate.DTW._fields == ("total", "length", "path_a", "path_b")
    assert evaluate.MCD._fields == ("mcd", "total", "length", "path_hyp", "path_ref")
    assert Evaluation._fields == ("mcd", "length", "hyp_len", "ref_len", "mel_hyp")
    assert list(inspect.signature(ops.dtw).parameters) == ["a", "b", "total", "length", "a_len", "b_len", "cols",
                                                           "path_a", "path_b", "ws"]
    assert list(inspect.signature(evaluate.dtw).parameters) == ["a", "a_len", "b", "b_len", "cols", "want_path"]
    assert list(inspect.signature(evaluate.mcd_dtw).parameters) == ["mel_hyp", "hyp_len", "mel_ref", "ref_len",
                                                                   "n_coef", "want_path"]
    sig = inspect.signature(TransformerTTS.evaluate).parameters
    assert list(sig) == ["self", "text", "text_len", "mel", "mel_len", "max_len", "stop_threshold", "prenet_dropout",
                         "n_coef", "want_path"]
    assert sig["prenet_dropout"].default is False and sig["n_coef"].default == 13 and sig["max_len"].default is None
    w = evaluate.dct_basis(80, 13)
    assert tuple(w.shape) == (14, 80) and abs(float((w.double() @ w.double().T)[3, 3]) - 1) < 1e-6
    with pytest.raises(ValueError):
        evaluate.mfcc(__import__("torch").zeros(1, 2, 80), n_coef=16)


def test_workspace_size(lib):
    ws = lib.load().tt2_dtw_workspace_size
    assert ws(16, 800, 800, 0) == 0
    assert ws(0, 800, 800, 1) == 0 and ws(4, 0, 800, 1) == 0 and ws(4, 800, 0, 1) == 0
    assert ws(1, 1, 1, 1) > 0
    assert ws(1, 2048, 2048, 1) >= 2048 * 2048 // 4   # 2 bits per cell
    for lo, hi in (((2, 100, 90), (2, 101, 90)), ((2, 100, 90), (2, 117, 90)), ((2, 100, 90), (2, 100, 91)),
                   ((2, 100, 90), (3, 100, 90))):
        assert ws(*lo, 1) <= ws(*hi, 1), (lo, hi)
    assert ws(2, 100, 90, 1) < ws(2, 117, 90, 1) and ws(2, 100, 90, 1) < ws(2, 100, 91, 1) < ws(3, 100, 91, 1)


def test_host_refusals(lib):
    """Requests refused with TT2_E_INVALID before any launch (there is no GPU here: a launch would
    fail otherwise than with E_INVALID, and the no-op cases return TT2_OK without one)."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    a = lib.DtwArgs()
    a.a = a.b = a.total = a.length = p
    a.a_ld = a.b_ld = 16
    a.batch, a.ta, a.tb, a.c0, a.c1 = 1, 8, 8, 1, 14

    def rc(**kw):
        b = lib.DtwArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        return L.tt2_dtw(ctypes.byref(b), None)

    E = lib.E_INVALID
    assert E == -1
    assert rc(ta=lib.DTW_MAX_FRAMES + 1) == E and rc(tb=lib.DTW_MAX_FRAMES + 1) == E
    assert rc(c0=0, c1=0) == E and rc(c0=5, c1=5) == E and rc(c0=6, c1=5) == E
    assert rc(c0=0, c1=33, a_ld=64, b_ld=64) == E
    assert rc(c0=-1, c1=8) == E
    assert rc(a_ld=13) == E and rc(b_ld=13) == E
    assert rc(batch=-1) == E
    assert rc(path_a=p) == E and rc(path_b=p) == E
    need = L.tt2_dtw_workspace_size(1, 8, 8, 1)
    assert need > 0
    assert rc(path_a=p, path_b=p) == E                                         # no workspace
    assert rc(path_a=p, path_b=p, workspace=p, workspace_bytes=need - 1) == E  # too small
    assert rc(total=None) == E and rc(length=None) == E
    assert b"tt2_dtw" in L.tt2_last_error()
    # batch = 0 is a successful no-op, also with a path and no workspace
    assert rc(batch=0) == 0 and rc(batch=0, path_a=p, path_b=p) == 0


def test_dtw_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and the struct's size, from a tiny host program."""
    structs = {"tt2_dtw_args": lib.DtwArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_frames value %d\\n", TT2_DTW_MAX_FRAMES);\n'
    prog += 'printf("max_feats value %d\\n", TT2_DTW_MAX_FEATS);\n'
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
        if name == "max_frames":
            assert int(val) == lib.DTW_MAX_FRAMES
        elif name == "max_feats":
            assert int(val) == lib.DTW_MAX_FEATS
        elif field == "size":
            assert ctypes.sizeof(structs[name]) == int(val), name
        else:
            assert getattr(structs[name], field).offset == int(val), (name, field)
        seen += 1
    assert seen == 2 + sum(1 + len(c._fields_) for c in structs.values())
