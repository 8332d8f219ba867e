"""CPU: the guided-attention entry points are exported and bound, and the ctypes structs of
tt2_attn_guide / tt2_guide_loss_args match the C layout (test_capi.py's approach, for the
structs it does not list).  No compute calls (no GPU here)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tt2_attn_fwd_guided", "tt2_attn_bwd_guided", "tt2_guided_attn_loss")


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_guided_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    for name in NEW + ("tt2_attn_guide", "tt2_guide_loss_args"):
        assert name in header, name
    bound = lib.load()
    assert bound.tt2_attn_fwd_guided.argtypes[1]._type_ is lib.AttnGuide
    assert bound.tt2_guided_attn_loss.argtypes[0]._type_ is lib.GuideLossArgs
    from tt2 import ops
    for fn in ("attn_fwd_guided", "attn_bwd_guided", "guided_attn_loss"):
        assert callable(getattr(ops, fn))


def test_guided_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and each struct's size, from a tiny host program."""
    structs = {"tt2_attn_guide": lib.AttnGuide, "tt2_guide_loss_args": lib.GuideLossArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_layers value %d\\n", TT2_GUIDE_MAX_LAYERS);\n'
    prog += "return 0;}\n"
    src, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(src, "w").write(prog)
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("host C compiler cannot include hip_runtime_api.h: " + r.stderr[-300:])
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
