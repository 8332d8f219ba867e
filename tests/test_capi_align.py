"""CPU: the alignment-statistics entry points are exported and bound, and the ctypes structs of
tt2_align_args / tt2_align_dur_args match the C layout (test_capi_guided.py's approach).  No
compute calls (no GPU here)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tt2_attn_align", "tt2_align_durations")


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_align_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    for name in NEW + ("tt2_align_args", "tt2_align_dur_args"):
        assert name in header, name
    bound = lib.load()
    assert bound.tt2_attn_align.argtypes[0]._type_ is lib.AlignArgs
    assert bound.tt2_align_durations.argtypes[0]._type_ is lib.AlignDurArgs
    from tt2 import ops
    for fn in ("attn_align", "align_durations"):
        assert callable(getattr(ops, fn))
    from tt2.model import AlignmentStats, Durations, TransformerTTS
    assert AlignmentStats._fields == ("pmax", "argmax", "focus", "layers")
    assert Durations._fields == ("durations", "head", "focus")
    for fn in ("alignment_stats", "durations"):
        assert callable(getattr(TransformerTTS, fn))


def test_align_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and each struct's size, from a tiny host program."""
    structs = {"tt2_align_args": lib.AlignArgs, "tt2_align_dur_args": lib.AlignDurArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_layers value %d\\n", TT2_GUIDE_MAX_LAYERS);\n'
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
        if name == "max_layers":
            assert int(val) == lib.GUIDE_MAX_LAYERS
        elif field == "size":
            assert ctypes.sizeof(structs[name]) == int(val), name
        else:
            assert getattr(structs[name], field).offset == int(val), (name, field)
        seen += 1
    assert seen == 1 + sum(1 + len(c._fields_) for c in structs.values())
