"""CPU: tt2_regulate_plan / _fwd / _bwd are exported and bound, the ctypes structs match the C layout
(test_capi_trim.py's approach), every host-side refusal and zero-size success behaves as the header
states, and the Python surface is as documented.  No compute calls (no GPU here)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tt2_regulate_plan", "tt2_regulate_fwd", "tt2_regulate_bwd")


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_regulate_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    bound = lib.load()
    for name in ENTRIES:
        assert hasattr(L, name) and name in lib.SIGNATURES and name in header, name
        assert getattr(bound, name).restype is ctypes.c_int
    for name in ("tt2_regulate_plan_args", "tt2_regulate_args", "TT2_REGULATE_MAX_PHONEMES"):
        assert name in header, name
    assert bound.tt2_regulate_plan.argtypes[0]._type_ is lib.RegulatePlanArgs
    assert bound.tt2_regulate_fwd.argtypes[0]._type_ is lib.RegulateArgs
    assert bound.tt2_regulate_bwd.argtypes[0]._type_ is lib.RegulateArgs
    assert lib.REGULATE_MAX_PHONEMES == 4096


def test_python_surface(lib):
    from tt2 import ops, regulate
    sig = inspect.signature(ops.regulate_plan).parameters
    assert list(sig) == ["durations", "n_out", "key_len", "ends", "index", "frames", "total"]
    assert all(sig[k].default is None for k in list(sig)[2:])
    assert list(inspect.signature(ops.regulate_fwd).parameters) == ["h", "index", "y"]
    assert list(inspect.signature(ops.regulate_bwd).parameters) == ["dy", "ends", "dh"]
    assert regulate.RegulatorPlan._fields == ("index", "ends", "frames", "total")
    assert regulate.Regulated._fields == ("out", "frames", "index")
    sig = inspect.signature(regulate.plan).parameters
    assert list(sig) == ["durations", "text_len", "max_frames"] and sig["text_len"].default is None and sig["max_frames"].default is None
    sig = inspect.signature(regulate.length_regulate).parameters
    assert list(sig) == ["h", "durations", "text_len", "max_frames", "plan"]
    assert all(sig[k].default is None for k in list(sig)[1:])
    assert list(inspect.signature(regulate.segment_sum).parameters) == ["values", "plan"]
    sig = inspect.signature(regulate.LengthRegulator.forward).parameters
    assert list(sig) == ["self", "h", "durations", "text_len", "max_frames"]
    assert sig["text_len"].default is None and sig["max_frames"].default is None
    sig = inspect.signature(regulate.round_durations).parameters
    assert list(sig) == ["log_d", "text_len", "alpha", "min_frames"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, 1.0, 0]
    import torch
    assert issubclass(regulate.LengthRegulator, torch.nn.Module) and not list(regulate.LengthRegulator().parameters())


def test_ops_refuse_before_the_c_call(lib):
    """ValueError for what the header refuses, raised on CPU tensors before anything touches a GPU."""
    import torch
    from tt2 import ops, regulate
    i32 = torch.int32
    d, e = torch.zeros(2, 5, dtype=i32), torch.zeros(2, 5, dtype=i32)
    bad_plans = [dict(durations=d.long(), n_out=4, ends=e), dict(durations=d, n_out=-1, ends=e), dict(durations=d, n_out=4),
                 dict(durations=d, n_out=4, ends=e[:, :4]), dict(durations=d, n_out=4, ends=e, index=torch.zeros(2, 3, dtype=i32)),
                 dict(durations=d, n_out=4, ends=e, frames=torch.zeros(3, dtype=i32)),
                 dict(durations=d, n_out=4, ends=e, key_len=torch.zeros(2, dtype=torch.int64)),
                 dict(durations=torch.zeros(1, 4097, dtype=i32), n_out=4, ends=torch.zeros(1, 4097, dtype=i32)),
                 dict(durations=d.t(), n_out=4, ends=torch.zeros(5, 2, dtype=i32)), dict(durations=d[0], n_out=4, ends=e),
                 dict(durations=d, n_out=4, ends=e)]                      # the last: well-formed, but not on a GPU
    for kw in bad_plans:
        with pytest.raises(ValueError, match="regulate_plan"):
            ops.regulate_plan(**kw)
    h, y, idx = torch.zeros(2, 5, 8), torch.zeros(2, 7, 8), torch.zeros(2, 7, dtype=i32)
    bad = [(h.half(), idx, y.half()), (h.bfloat16(), idx, y), (h, idx, torch.zeros(2, 7, 9)), (h, idx, torch.zeros(3, 7, 8)),
           (h, idx[:, :6], y), (h, idx.long(), y), (h[0], idx, y), (h, idx, y.transpose(1, 2)),
           (torch.zeros(2, 4097, 8), idx, y), (h, idx, torch.zeros(1, 7, 8).expand(2, 7, 8)), (h, idx, y)]
    for args in bad:
        with pytest.raises(ValueError, match="regulate_fwd"):
            ops.regulate_fwd(*args)
    dy, dh, ends = y, h, torch.zeros(2, 5, dtype=i32)
    for args in [(dy.double(), ends, dh.double()), (dy, ends[:, :4], dh), (dy, ends, torch.zeros(2, 4097, 8)),
                 (dy, ends, torch.zeros(2, 5, 4)), (dy, ends, dh)]:
        with pytest.raises(ValueError, match="regulate_bwd"):
            ops.regulate_bwd(*args)
    with pytest.raises(ValueError):
        regulate.plan(torch.zeros(2, 5))
    with pytest.raises(ValueError):
        regulate.plan(torch.zeros(2, 5, dtype=i32))                        # not on a GPU
    with pytest.raises(ValueError):
        regulate.length_regulate(h)
    p = regulate.RegulatorPlan(idx, ends, torch.zeros(2, dtype=i32), torch.zeros(2, dtype=i32))
    with pytest.raises(ValueError):
        regulate.length_regulate(h, durations=d, plan=p)
    with pytest.raises(ValueError):
        regulate.length_regulate(h, plan=p, max_frames=7)
    with pytest.raises(ValueError):
        regulate.segment_sum(torch.zeros(2, 8, 8), p)


def test_host_refusals_and_zero_sizes(lib):
    """Requests refused with TT2_E_INVALID before any launch (there is no GPU here: a launch would
    fail otherwise than with E_INVALID), and the zero-size calls return TT2_OK without one."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    ptr = ctypes.addressof(buf)
    E = lib.E_INVALID
    big = 2 ** 31 - 1
    fns = {"tt2_regulate_plan": L.tt2_regulate_plan, "tt2_regulate_fwd": L.tt2_regulate_fwd,
           "tt2_regulate_bwd": L.tt2_regulate_bwd}

    def refused(name, a, kw):
        b = type(a).from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        # something else first, so that the message read afterwards belongs to this call
        assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()
        rc = fns[name](ctypes.byref(b), None)
        return rc, L.tt2_last_error()

    def check(name, a, refusals, successes):
        for kw in refusals:
            rc, msg = refused(name, a, kw)
            assert rc == E and msg.startswith(name.encode() + b":"), (name, kw, rc, msg)
        for kw in successes:
            assert refused(name, a, kw)[0] == 0, (name, kw)
        assert fns[name](None, None) == E and L.tt2_last_error().startswith(name.encode() + b":")

    a = lib.RegulatePlanArgs()
    a.durations = a.key_len = a.ends = a.index = a.frames = a.total = ptr
    a.dur_ld, a.ends_ld, a.index_ld = 128, 130, 800
    a.batch, a.tx, a.n_out = 2, 128, 800
    check("tt2_regulate_plan", a,
          [dict(batch=-1), dict(tx=-1), dict(n_out=-1), dict(tx=4097, dur_ld=4097, ends_ld=4097),
           dict(dur_ld=127), dict(ends_ld=127), dict(index_ld=799), dict(dur_ld=-1), dict(durations=None), dict(ends=None),
           dict(batch=big, n_out=1025, index_ld=1025),                  # two work groups per utterance
           dict(batch=0, tx=-1), dict(batch=0, dur_ld=127), dict(batch=0, tx=4097, dur_ld=4097, ends_ld=4097)],
          [dict(batch=0), dict(batch=0, durations=None, ends=None, index=None, frames=None, total=None, key_len=None),
           dict(batch=0, tx=4096, dur_ld=4096, ends_ld=4096), dict(batch=0, n_out=big, index_ld=big),
           dict(batch=0, index=None, index_ld=0), dict(batch=0, tx=0, n_out=0),
           # nothing to write at all: tx = 0 and no frames, total or index rows
           dict(tx=0, n_out=0, frames=None, total=None), dict(tx=0, frames=None, total=None, index=None, durations=None, ends=None)])

    a = lib.RegulateArgs()
    a.src = a.dst = a.map = ptr
    a.src_ld, a.src_bs, a.dst_ld, a.dst_bs, a.map_ld = 512, 128 * 512, 520, 800 * 520, 800
    a.batch, a.tx, a.n_out, a.dim, a.dtype = 2, 128, 800, 512, lib.DT_BF16
    common = [dict(batch=-1), dict(tx=-1), dict(n_out=-1), dict(dim=-1), dict(tx=4097), dict(src_ld=511), dict(dst_ld=511),
              dict(src_ld=-1), dict(dtype=lib.DT_F16), dict(dtype=3), dict(dtype=-1), dict(dst=None), dict(src=None),
              dict(map=None), dict(batch=0, dim=-1), dict(batch=0, dtype=2), dict(batch=0, src_ld=1)]
    check("tt2_regulate_fwd", a,
          common + [dict(map_ld=799), dict(n_out=0, map_ld=-1), dict(dim=0, tx=4097), dict(n_out=0, dst_ld=1),
                    dict(batch=big, n_out=17),                          # 16 rows per work group at dim 512
                    dict(batch=big, n_out=big, map_ld=big, dim=1, dtype=lib.DT_F32)],
          [dict(batch=0), dict(n_out=0), dict(dim=0), dict(batch=0, src=None, dst=None, map=None),
           dict(n_out=0, src=None, dst=None, map=None, map_ld=0), dict(dim=0, src=None, dst=None, map=None),
           dict(batch=0, dtype=lib.DT_F32), dict(n_out=0, tx=0), dict(batch=0, tx=4096),
           dict(map_ld=128, n_out=0)])
    a.map_ld = 128
    a.src_ld, a.src_bs, a.dst_ld, a.dst_bs = 520, 800 * 520, 512, 128 * 512
    check("tt2_regulate_bwd", a,
          common + [dict(map_ld=127), dict(tx=0, map_ld=-1), dict(dim=0, tx=4097), dict(tx=0, dst_ld=1),
                    dict(batch=big, tx=5),                              # 4 phonemes per work group at dim 512
                    dict(batch=big, tx=4096, map_ld=4096, dim=1, dtype=lib.DT_F32)],
          [dict(batch=0), dict(tx=0), dict(dim=0), dict(batch=0, src=None, dst=None, map=None),
           dict(tx=0, src=None, dst=None, map=None, map_ld=0), dict(dim=0, src=None, dst=None, map=None),
           dict(tx=0, n_out=0), dict(batch=0, n_out=0), dict(batch=big, tx=0), dict(batch=0, tx=4096, map_ld=4096)])


def test_regulate_struct_layouts_match_c(lib, tmp_path):
    """Every field's offset and both structs' sizes, from a tiny host program."""
    structs = {"tt2_regulate_plan_args": lib.RegulatePlanArgs, "tt2_regulate_args": lib.RegulateArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_phonemes value %d\\n", TT2_REGULATE_MAX_PHONEMES);\n'
    prog += "return 0;}\n"
    # skipped only where the program cannot be built at all; a compile error is a failure
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc or no hip_runtime_api.h on this machine")
    src, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(src, "w").write(prog)
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    consts = {"max_phonemes": lib.REGULATE_MAX_PHONEMES}
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
