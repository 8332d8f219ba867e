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


# ------------------------------------------------------------------ refusals (no launch: host buffers)
def _fill(struct, fields, buf):
    """A struct from keyword -> value; "buffer" stands for a non-null host pointer."""
    s = struct()
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(s, k)[i] = ctypes.addressof(buf) if x == "buffer" else x
        else:
            setattr(s, k, ctypes.addressof(buf) if v == "buffer" else v)
    return s


P = "buffer"
ATTN_VALID = dict(q=P, k=P, v=P, o=P, dout=P, o_out=P, dq=P, dk=P, dv=P, lse=P, delta=P, q_ld=192, k_ld=192, v_ld=192,
                  o_ld=192, do_ld=192, dq_ld=192, dk_ld=192, dv_ld=192, key_len=None, batch=2, heads=3, head_dim=64,
                  tq=33, tk=64, causal=0, dtype=1, scale=0.125, variant=0, parts=0)
GUIDE_VALID = dict(q_len=None, rows=P, coef=P, sigma=0.4, heads=2)
# check_guide's four refusals: (changes of the attention args, changes of the guide or None for no guide)
GUIDE_REFUSALS = [({}, None), (dict(causal=1), {}), ({}, dict(rows=None)), ({}, dict(sigma=0.0)), ({}, dict(sigma=-0.4)),
                  ({}, dict(sigma=float("nan"))), ({}, dict(heads=-1)), ({}, dict(heads=4))]
LOSS_VALID = dict(rows=[P, P], key_len=None, q_len=None, loss_out=None, term=P, coef=P, n_layers=2, batch=2, heads=3,
                  guide_heads=2, tq=33, tk=64, scale=10.0, grad_scale=1.0)
LOSS_REFUSALS = [dict(term=None), dict(coef=None),                                   # "term / coef"
                 dict(n_layers=17), dict(n_layers=-1),                               # "too many layers"
                 dict(batch=-1), dict(tq=-1), dict(tk=-1), dict(heads=0), dict(guide_heads=-1), dict(guide_heads=4),
                 dict(heads=3, guide_heads=0, tq=2 ** 30),                           # "shape": heads * tq in 32 bits
                 dict(rows=[P, None]), dict(rows=[None, P])]                         # "rows buffer missing"


def test_every_stated_refusal(lib):
    """Valid arguments plus one bad field per row: TT2_E_INVALID with the entry's name in
    tt2_last_error(), before any launch (the buffers are host memory)."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    E = lib.E_INVALID

    def refused(name, *args):
        assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()     # so the message is this call's
        assert getattr(L, name)(*args, None) == E, (name, args)
        assert name.encode() in L.tt2_last_error(), (name, L.tt2_last_error())

    for name in ("tt2_attn_fwd_guided", "tt2_attn_bwd_guided"):
        cases = GUIDE_REFUSALS + ([({}, dict(coef=None))] if "bwd" in name else [])
        for akw, gkw in cases:
            a = _fill(lib.AttnArgs, dict(ATTN_VALID, **akw), buf)
            g = None if gkw is None else ctypes.byref(_fill(lib.AttnGuide, dict(GUIDE_VALID, **gkw), buf))
            refused(name, ctypes.byref(a), g)
    refused("tt2_guided_attn_loss", None)
    for kw in LOSS_REFUSALS:
        assert set(kw) <= set(LOSS_VALID)
        refused("tt2_guided_attn_loss", ctypes.byref(_fill(lib.GuideLossArgs, dict(LOSS_VALID, **kw), buf)))


def test_header_states_the_refusals():
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    sec = header[header.index("Guided attention (diagonal loss"):header.index("Alignment statistics of forwards")]
    sec = " ".join(sec.replace("*", " ").split())
    for phrase in ("a NULL guide", "causal != 0", "rows NULL", "coef NULL in the backward", "sigma <= 0 or NaN",
                   "heads < 0 or heads > the attention's heads", "NULL args, term or coef",
                   "n_layers < 0 or n_layers > TT2_GUIDE_MAX_LAYERS", "batch, tq or tk < 0", "heads <= 0",
                   "guide_heads < 0 or guide_heads > heads", "heads tq above INT32_MAX", "a NULL rows[l] with l < n_layers",
                   "parts = 2 alone runs no dQ block and leaves the scratch untouched"):
        assert phrase in sec, phrase
    assert sec.count("Refused (TT2_E_INVALID") == 2
