"""CPU: tt2_forward_sum_fwd / _bwd / _path and their workspace queries are exported and bound, the
ctypes struct matches the C layout (test_capi_trim.py's approach), every host-side refusal and
zero-size success behaves as the header states, and the Python surface is as documented.  No compute
calls (no GPU here)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tt2_forward_sum_fwd", "tt2_forward_sum_bwd", "tt2_forward_sum_path")
QUERIES = ("tt2_forward_sum_bwd_workspace_size", "tt2_forward_sum_path_workspace_size")


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_forward_sum_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    bound = lib.load()
    for name in ENTRIES + QUERIES:
        assert hasattr(L, name) and name in lib.SIGNATURES and name in header, name
    for name in ENTRIES:
        assert getattr(bound, name).restype is ctypes.c_int
        assert getattr(bound, name).argtypes[0]._type_ is lib.ForwardSumArgs
    for name in QUERIES:
        assert getattr(bound, name).restype is ctypes.c_size_t
    for name in ("tt2_forward_sum_args", "TT2_FSUM_MAX_KEYS", "TT2_FSUM_MAX_FRAMES"):
        assert name in header, name
    assert (lib.FSUM_MAX_KEYS, lib.FSUM_MAX_FRAMES) == (512, 4096) == (lib.MONO_MAX_KEYS, lib.MONO_MAX_FRAMES)


def test_workspace_queries(lib):
    L = lib.load()
    bwd, path = L.tt2_forward_sum_bwd_workspace_size, L.tt2_forward_sum_path_workspace_size
    assert bwd(16, 800, 128) == 16 * 800 * 128 * 4 and bwd(2, 10, 129) == 2 * 10 * 256 * 4 and bwd(1, 1, 512) == 512 * 4
    for zero in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (1, 1, 513)):
        assert bwd(*zero) == 0 and path(*zero) == 0
    # the move bits stay in LDS up to 4096 / 1536 / 256 frames at 128 / 256 / 512 keys
    assert path(3, 4096, 128) == 0 and path(3, 1536, 256) == 0 and path(3, 256, 512) == 0
    assert path(3, 1537, 256) == 3 * 1537 * 4 * 8 and path(3, 257, 512) == 3 * 257 * 8 * 8


def test_python_surface(lib):
    import torch
    from tt2 import forward_sum as FS, ops
    assert list(inspect.signature(ops.forward_sum_fwd).parameters) == ["scores", "loss", "lse", "alpha", "q_len", "key_len"]
    assert list(inspect.signature(ops.forward_sum_bwd).parameters) == [
        "scores", "lse", "alpha", "dscores", "gamma", "grad_loss", "q_len", "key_len", "workspace"]
    assert list(inspect.signature(ops.forward_sum_path).parameters) == [
        "scores", "path", "durations", "logp", "q_len", "key_len", "workspace"]
    sig = inspect.signature(FS.forward_sum_loss).parameters
    assert list(sig) == ["scores", "text_len", "mel_len", "reduction"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, None, "mean"]
    for fn in (FS.posterior, FS.best_path):
        assert list(inspect.signature(fn).parameters) == ["scores", "text_len", "mel_len"]
    sig = inspect.signature(FS.beta_binomial_prior).parameters
    assert list(sig) == ["text_len", "mel_len", "tx", "ty", "scaling"] and sig["scaling"].default == 1.0
    assert FS.ForwardSum._fields == ("loss", "gamma") and FS.HardAlignment._fields == ("durations", "path", "logp")
    from tt2.model import MonotonicAlignment
    assert FS.HardAlignment._fields[:2] == MonotonicAlignment._fields[:2]
    assert issubclass(FS.ForwardSumLoss, torch.nn.Module) and not list(FS.ForwardSumLoss().parameters())
    assert list(inspect.signature(FS.ForwardSumLoss.forward).parameters) == ["self", "scores", "text_len", "mel_len"]
    with pytest.raises(ValueError):
        FS.ForwardSumLoss(reduction="avg")


def test_wrappers_refuse_before_the_c_call(lib):
    """ValueError for what the header refuses, raised on CPU tensors before anything touches a GPU."""
    import torch
    from tt2 import forward_sum as FS, ops
    f32, i32 = torch.float32, torch.int32
    s, loss, lse, alpha = torch.zeros(2, 7, 5), torch.zeros(2), torch.zeros(2, 7), torch.zeros(2, 7, 5)
    bad = [dict(scores=s.double(), loss=loss, lse=lse), dict(scores=s[0], loss=loss, lse=lse),
           dict(scores=s.transpose(1, 2), loss=loss, lse=lse), dict(scores=s, loss=torch.zeros(3), lse=lse),
           dict(scores=s, loss=loss, lse=torch.zeros(2, 6)), dict(scores=s, loss=loss, lse=lse, alpha=torch.zeros(2, 7, 4)),
           dict(scores=s, loss=loss, lse=lse, q_len=torch.zeros(2, dtype=torch.int64)),
           dict(scores=s, loss=loss, lse=lse, key_len=torch.zeros(3, dtype=i32)),
           dict(scores=torch.zeros(1, 2, 513), loss=torch.zeros(1), lse=torch.zeros(1, 2)),
           dict(scores=torch.zeros(1, 4097, 2), loss=torch.zeros(1), lse=torch.zeros(1, 4097)),
           dict(scores=s, loss=None, lse=lse), dict(scores=s, loss=loss, lse=lse, alpha=alpha)]   # the last: well-formed, not on a GPU
    for kw in bad:
        with pytest.raises(ValueError, match="forward_sum_fwd"):
            ops.forward_sum_fwd(**kw)
    d = torch.zeros(2, 7, 5)
    bad = [dict(), dict(dscores=d.double()), dict(dscores=torch.zeros(2, 7, 4)), dict(gamma=torch.zeros(2, 6, 5)),
           dict(dscores=torch.zeros(1, 7, 5).expand(2, 7, 5)), dict(dscores=d, grad_loss=torch.zeros(3)),
           dict(dscores=d, grad_loss=torch.zeros(2, dtype=torch.float64)), dict(dscores=d, gamma=d.clone())]
    for kw in bad:
        with pytest.raises(ValueError, match="forward_sum_bwd"):
            ops.forward_sum_bwd(s, lse, alpha, **kw)
    with pytest.raises(ValueError, match="forward_sum_bwd"):
        ops.forward_sum_bwd(s, lse, None, dscores=d)
    path, dur, logp = torch.zeros(2, 7, dtype=i32), torch.zeros(2, 5, dtype=i32), torch.zeros(2)
    for args in [(path.long(), dur, logp), (path, dur[:, :4], logp), (path, dur, None), (path[:, :6], dur, logp),
                 (path, dur, logp.double()), (path, dur, logp)]:
        with pytest.raises(ValueError, match="forward_sum_path"):
            ops.forward_sum_path(s, *args)
    for fn in (FS.forward_sum_loss, FS.posterior, FS.best_path):
        for x in (s, s.double(), s[0], torch.zeros(2, 2, 7, 5)):
            with pytest.raises(ValueError):
                fn(x)
    with pytest.raises(ValueError):
        FS.forward_sum_loss(s, reduction="avg")
    assert f32 == alpha.dtype


def test_host_refusals_and_zero_sizes(lib):
    """Requests refused with TT2_E_INVALID before any launch (there is no GPU here: a launch would
    fail otherwise than with E_INVALID), and the zero-size calls that need no launch return TT2_OK."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    ptr = (ctypes.addressof(buf) + 15) & ~15
    E = lib.E_INVALID
    big = 2 ** 31 - 1
    fns = {n: getattr(L, n) for n in ENTRIES}

    def run(name, a, kw):
        b = type(a).from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        # something else first, so that the message read afterwards belongs to this call
        assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()
        rc = fns[name](ctypes.byref(b), None)
        return rc, L.tt2_last_error()

    a = lib.ForwardSumArgs()
    for f in ("scores", "q_len", "key_len", "loss", "lse", "alpha", "grad_loss", "dscores", "gamma", "path", "durations",
              "logp", "workspace"):
        setattr(a, f, ptr)
    a.workspace_bytes = 2 ** 40
    a.s_ld, a.s_bs, a.a_ld, a.d_ld, a.d_bs, a.g_ld, a.g_bs = 130, 800 * 130, 128, 129, 800 * 129, 128, 800 * 128
    a.batch, a.tq, a.tk = 2, 800, 128
    common = [dict(batch=-1), dict(tq=-1), dict(tk=-1), dict(tk=513, s_ld=513, a_ld=513, d_ld=513, g_ld=513),
              dict(tq=4097), dict(s_ld=127), dict(s_ld=-1), dict(scores=None), dict(batch=0, tk=-1), dict(batch=0, s_ld=1),
              dict(batch=0, tq=4097)]
    refusals = {
        "tt2_forward_sum_fwd": common + [dict(a_ld=127), dict(loss=None), dict(lse=None), dict(batch=0, a_ld=3)],
        "tt2_forward_sum_bwd": common + [dict(a_ld=127), dict(d_ld=127), dict(g_ld=127), dict(alpha=None), dict(lse=None),
                                         dict(dscores=None, gamma=None), dict(workspace=None), dict(workspace=ptr + 4),
                                         dict(workspace_bytes=2 * 800 * 128 * 4 - 1), dict(batch=big, tq=5),
                                         dict(batch=0, d_ld=3)],
        "tt2_forward_sum_path": common + [dict(path=None), dict(durations=None), dict(logp=None),
                                          dict(tq=1537, tk=256, s_ld=256, workspace=None),
                                          dict(tq=1537, tk=256, s_ld=256, workspace_bytes=2 * 1537 * 32 - 1),
                                          dict(tq=1537, tk=256, s_ld=256, workspace=ptr + 4)],
    }
    successes = {
        "tt2_forward_sum_fwd": [dict(batch=0), dict(batch=0, scores=None, loss=None, lse=None, alpha=None),
                                dict(batch=0, tq=4096, tk=512, s_ld=512, a_ld=512), dict(batch=0, alpha=None, a_ld=0)],
        "tt2_forward_sum_bwd": [dict(batch=0), dict(tq=0), dict(tk=0), dict(tq=0, scores=None, lse=None, alpha=None, dscores=None, gamma=None),
                                dict(batch=0, workspace=None, workspace_bytes=0), dict(tk=0, workspace=None, s_ld=0, a_ld=0, d_ld=0, g_ld=0),
                                dict(batch=0, dscores=None, d_ld=0, gamma=None, g_ld=0)],
        "tt2_forward_sum_path": [dict(batch=0), dict(batch=0, scores=None, path=None, durations=None, logp=None),
                                 dict(batch=0, tq=4096, tk=512, s_ld=512)],
    }
    for name in ENTRIES:
        for kw in refusals[name]:
            rc, msg = run(name, a, kw)
            assert rc == E and msg.startswith(name.encode() + b":"), (name, kw, rc, msg)
        for kw in successes[name]:
            assert run(name, a, kw)[0] == 0, (name, kw)
        assert fns[name](None, None) == E and L.tt2_last_error().startswith(name.encode() + b":")


def test_forward_sum_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and the struct's size, from a tiny host program."""
    structs = {"tt2_forward_sum_args": lib.ForwardSumArgs}
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    for name, cls in structs.items():
        prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        for field, _ in cls._fields_:
            prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_keys value %d\\n", TT2_FSUM_MAX_KEYS);\nprintf("max_frames value %d\\n", TT2_FSUM_MAX_FRAMES);\n'
    prog += "return 0;}\n"
    # skipped only where the program cannot be built at all; a compile error is a failure
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc or no hip_runtime_api.h on this machine")
    src, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(src, "w").write(prog)
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    consts = {"max_keys": lib.FSUM_MAX_KEYS, "max_frames": lib.FSUM_MAX_FRAMES}
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
    assert seen == 2 + sum(1 + len(c._fields_) for c in structs.values())
