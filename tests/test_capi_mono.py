"""CPU: the monotonic-alignment entry points are exported and bound, the ctypes struct of
tt2_align_mono_args matches the C layout (test_capi_align.py's approach), and the Python surface
is as documented.  No compute calls (no GPU here)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tt2_align_monotonic_workspace_size", "tt2_align_monotonic")


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_mono_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    for name in NEW + ("tt2_align_mono_args", "TT2_MONO_MAX_KEYS"):
        assert name in header, name
    bound = lib.load()
    assert bound.tt2_align_monotonic.argtypes[0]._type_ is lib.AlignMonoArgs
    assert bound.tt2_align_monotonic_workspace_size.restype is ctypes.c_size_t
    assert lib.MONO_MAX_KEYS >= 512


def test_python_surface(lib):
    from tt2 import data, ops
    from tt2.engine import TTSEngine
    from tt2.model import Durations, MonotonicAlignment, TransformerTTS
    assert MonotonicAlignment._fields == ("durations", "path", "head", "focus", "logp")
    assert Durations._fields == ("durations", "head", "focus")   # unchanged
    sig = inspect.signature(ops.align_monotonic)
    assert list(sig.parameters) == ["qs", "ks", "lses", "path", "durations", "logp", "q_ld", "k_ld", "batch", "heads",
                                    "tq", "tk", "key_len", "q_len", "sel", "head", "scale", "variant", "ws"]
    assert list(inspect.signature(TTSEngine.align_monotonic).parameters) == ["self", "A", "layers", "head"]
    assert inspect.signature(TransformerTTS.monotonic_durations) .parameters.keys() == \
        inspect.signature(TransformerTTS.durations).parameters.keys()
    assert inspect.signature(data.extract_durations).parameters["method"].default == "argmax"


def test_workspace_size_and_host_refusals(lib):
    """Host-side logic only: the size query, and requests refused before any launch."""
    L = lib.load()
    ws = L.tt2_align_monotonic_workspace_size
    assert ws(16, 800, 128) == 0                 # the benchmark shape keeps its move bits in LDS
    assert ws(4, 2000, 512) == 4 * 2000 * 16 * 4  # tq rows of 512 / 32 words each
    assert ws(0, 800, 128) == 0 and ws(4, 0, 128) == 0
    a = lib.AlignMonoArgs()
    buf = (ctypes.c_char * 64)()
    for i in range(1):
        a.q[i] = a.k[i] = a.lse[i] = ctypes.addressof(buf)
    a.path = a.durations = a.logp = ctypes.addressof(buf)
    a.q_ld = a.k_ld = 64
    a.n_layers, a.batch, a.heads, a.head_dim, a.tq, a.tk, a.dtype, a.scale = 1, 1, 1, 64, 8, 8, lib.DT_BF16, 0.125

    def refused(**kw):
        b = lib.AlignMonoArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        rc = L.tt2_align_monotonic(ctypes.byref(b), None)
        return rc == lib.E_INVALID if hasattr(lib, "E_INVALID") else rc != 0

    assert refused(tk=lib.MONO_MAX_KEYS + 1)
    assert refused(tq=lib.MONO_MAX_FRAMES + 1)
    assert refused(causal=1)
    assert refused(scale=0.0)
    assert refused(head_dim=32)
    assert refused(n_layers=0) and refused(n_layers=17)
    assert refused(variant=2)
    assert refused(q_ld=60)
    assert refused(sel_head=1)
    assert refused(tq=2000, tk=512)   # needs a workspace, none given
    assert refused(tq=2000, tk=512, workspace=ctypes.addressof(buf), workspace_bytes=64)


def test_mono_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and the struct's size, from a tiny host program."""
    structs = {"tt2_align_mono_args": lib.AlignMonoArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_keys value %d\\n", TT2_MONO_MAX_KEYS);\n'
    prog += 'printf("max_frames value %d\\n", TT2_MONO_MAX_FRAMES);\n'
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
        if name == "max_keys":
            assert int(val) == lib.MONO_MAX_KEYS
        elif name == "max_frames":
            assert int(val) == lib.MONO_MAX_FRAMES
        elif field == "size":
            assert ctypes.sizeof(structs[name]) == int(val), name
        else:
            assert getattr(structs[name], field).offset == int(val), (name, field)
        seen += 1
    assert seen == 2 + sum(1 + len(c._fields_) for c in structs.values())
