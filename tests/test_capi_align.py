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


# ------------------------------------------------------------------ refusals (no launch: host buffers)
P = "buffer"
ALIGN_VALID = dict(q=[P, P], k=[P, P], lse=[P, P], q_ld=192, k_ld=1152, key_len=None, q_len=None, pmax=P, amax=P,
                   n_layers=2, batch=2, heads=3, head_dim=64, tq=33, tk=64, dtype=1, causal=0, scale=0.125, variant=0)
ALIGN_REFUSALS = [dict(head_dim=32), dict(causal=1), dict(n_layers=17), dict(n_layers=-1),
                  dict(dtype=2), dict(dtype=-1),
                  dict(batch=-1), dict(heads=0), dict(tq=-1), dict(tk=-1), dict(scale=0.0), dict(scale=-0.125),
                  dict(scale=float("nan")), dict(batch=65536, heads=65536, q_ld=2 ** 22, k_ld=2 ** 22),
                  dict(q_ld=193), dict(k_ld=1153), dict(q_ld=128), dict(k_ld=184),
                  dict(pmax=None), dict(amax=None),
                  dict(q=[P, None]), dict(k=[None, P]), dict(lse=[P, None]),
                  dict(tq=2 ** 20, q_ld=2048), dict(tk=2 ** 20, k_ld=2048), dict(variant=3, tk=2 ** 19, k_ld=4096),   # 2 GiB
                  dict(variant=1, batch=21846), dict(dtype=0, batch=21846)]                                        # 65535 pairs
DUR_VALID = dict(pmax=P, amax=P, key_len=None, q_len=None, focus=P, sel=P, sel_focus=P, durations=P, n_layers=2, batch=2,
                 heads=3, tq=33, tk=64, mode=0, sel_layer=0, sel_head=0)
DUR_REFUSALS = [dict(pmax=None), dict(amax=None), dict(focus=None), dict(sel=None), dict(sel_focus=None), dict(durations=None),
                dict(n_layers=0), dict(n_layers=17), dict(n_layers=-1),
                dict(batch=-1), dict(heads=0), dict(tq=-1), dict(tk=-1), dict(n_layers=5, heads=205),          # 1025 pairs
                dict(mode=2), dict(mode=-1),
                dict(mode=1, sel_layer=2), dict(mode=1, sel_layer=-1), dict(mode=1, sel_head=3), dict(mode=1, sel_head=-1)]


def _fill(struct, fields, buf):
    s = struct()
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(s, k)[i] = ctypes.addressof(buf) if x == P else x
        else:
            setattr(s, k, ctypes.addressof(buf) if v == P else v)
    return s


def test_every_stated_refusal(lib):
    """Valid arguments plus one bad field per row: TT2_E_INVALID with the entry's name in
    tt2_last_error().  The 2 GiB span and the 65535-pair limit are reached with dummy non-null
    pointers: both are refused before any launch."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    E = lib.E_INVALID
    for name, struct, valid, refusals in (("tt2_attn_align", lib.AlignArgs, ALIGN_VALID, ALIGN_REFUSALS),
                                          ("tt2_align_durations", lib.AlignDurArgs, DUR_VALID, DUR_REFUSALS)):
        for kw in [None] + refusals:
            assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()     # so the message is this call's
            if kw is None:
                rc = getattr(L, name)(None, None)
            else:
                assert set(kw) <= set(valid), (name, kw)
                rc = getattr(L, name)(ctypes.byref(_fill(struct, dict(valid, **kw), buf)), None)
            assert rc == E, (name, kw)
            assert name.encode() in L.tt2_last_error(), (name, kw, L.tt2_last_error())
    assert 21846 * 3 > 65535 and 5 * 205 == 1025
    # the largest shapes inside the limits pass the same checks: 1024 pairs with no utterance, 65535 pairs with no row
    assert L.tt2_align_durations(ctypes.byref(_fill(lib.AlignDurArgs, dict(DUR_VALID, n_layers=16, heads=64, batch=0), buf)), None) == 0
    assert L.tt2_attn_align(ctypes.byref(_fill(lib.AlignArgs, dict(ALIGN_VALID, variant=1, batch=21845, tq=0), buf)), None) == 0


def test_header_states_the_refusals():
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    sec = header[header.index("Alignment statistics of forwards"):header.index("Monotonic alignment search")]
    sec = " ".join(sec.replace("*", " ").split())
    for phrase in ("head_dim != 64", "causal != 0", "n_layers < 0 or n_layers > TT2_GUIDE_MAX_LAYERS",
                   "a dtype other than bf16 or f32", "scale <= 0 or NaN", "batch heads above INT32_MAX",
                   "no multiple of 16 bytes or is below heads 64", "NULL pmax or amax",
                   "a NULL q[l], k[l] or lse[l] with l < n_layers", "spanning more than 2 GiB",
                   "more than 65535 (batch, head) pairs",
                   "a NULL pmax, amax, focus, sel, sel_focus or durations", "n_layers < 1 or n_layers > TT2_GUIDE_MAX_LAYERS",
                   "n_layers heads above 1024", "a mode other than 0 or 1", "a sel_layer outside [0, n_layers)",
                   "a sel_head outside [0, heads)", "counts nowhere", "rows n >= Ty_b are not read"):
        assert phrase in sec, phrase
    assert sec.count("Refused (TT2_E_INVALID") == 2
