"""CPU: tt2_gauss_upsample_fwd / _bwd and the workspace size are exported and bound, the ctypes struct
matches the C layout (test_capi_regulate.py's approach), every host-side refusal and zero-size success
behaves as the header states, and the Python surface is as documented.  No compute calls (no GPU
here)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tt2_gauss_upsample_fwd", "tt2_gauss_upsample_bwd")


@pytest.fixture(scope="module")
def lib():
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


def test_upsample_symbols_exported_and_bound(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tt2_capi.h")).read()
    bound = lib.load()
    for name in ENTRIES:
        assert hasattr(L, name) and name in lib.SIGNATURES and name in header, name
        assert getattr(bound, name).restype is ctypes.c_int
        assert getattr(bound, name).argtypes[0]._type_ is lib.GaussUpsampleArgs
    name = "tt2_gauss_upsample_bwd_workspace_size"
    assert hasattr(L, name) and name in lib.SIGNATURES and name in header
    assert bound.tt2_gauss_upsample_bwd_workspace_size.restype is ctypes.c_size_t
    for name in ("tt2_gauss_upsample_args", "TT2_UPSAMPLE_MAX_DIM"):
        assert name in header, name
    assert lib.UPSAMPLE_MAX_DIM == 512 and lib.UPSAMPLE_MAX_DIM >= 512
    size = bound.tt2_gauss_upsample_bwd_workspace_size
    assert size(16, 128, 800, 512) >= 16 * 800 * 4 and size(16, 128, 800, 512) % 16 == 0
    assert size(0, 128, 800, 512) == 0 and size(16, 128, 0, 512) == 0 and size(16, 0, 800, 512) == 0
    assert size(16, 128, 800, 512) == 51200 + 7 * 16 * 128 * 512 * 4 + 7 * 16 * 3 * 128 * 4     # delta, 7 partials of dh and of the sums
    assert size(16, 128, 128, 512) == 16 * 128 * 4                         # four frame tiles: one work group, no partials


def test_python_surface(lib):
    import torch
    from tt2 import ops, upsample
    sig = inspect.signature(ops.gauss_upsample_fwd).parameters
    assert list(sig) == ["h", "center", "prec", "y", "lse", "bias", "q_len", "key_len", "offset"]
    assert [sig[k].default for k in list(sig)[5:]] == [None, None, None, 0.0]
    sig = inspect.signature(ops.gauss_upsample_bwd).parameters
    assert list(sig) == ["h", "center", "prec", "y", "lse", "dy", "dh", "dcenter", "dprec", "dbias", "bias", "q_len",
                         "key_len", "offset", "workspace"]
    assert [sig[k].default for k in list(sig)[6:]] == [None] * 7 + [0.0, None]
    assert upsample.Upsampled._fields == ("out", "frames")
    sig = inspect.signature(upsample.centers).parameters
    assert list(sig) == ["durations", "text_len"] and sig["text_len"].default is None
    sig = inspect.signature(upsample.gaussian_upsample).parameters
    assert list(sig) == ["h", "durations", "text_len", "mel_len", "max_frames", "delta", "sigma", "offset"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, None, None, 0.1, None, 0.0]
    sig = inspect.signature(upsample.GaussianUpsampling.__init__).parameters
    assert list(sig) == ["self", "delta", "offset"] and sig["delta"].default == 0.1 and sig["offset"].default == 0.0
    sig = inspect.signature(upsample.GaussianUpsampling.forward).parameters
    assert list(sig) == ["self", "h", "durations", "text_len", "mel_len", "max_frames"]
    assert issubclass(upsample.GaussianUpsampling, torch.nn.Module) and not list(upsample.GaussianUpsampling().parameters())


def test_centers_is_torch_and_differentiable(lib):
    import torch
    from tt2 import upsample
    d = torch.tensor([[2, 0, 3, 1], [1, 1, 9, 9]], dtype=torch.int32)
    c = upsample.centers(d, torch.tensor([4, 2]))
    assert c.dtype == torch.float32 and c.tolist() == [[1.0, 2.0, 3.5, 5.5], [0.5, 1.5, 0.0, 0.0]]
    assert upsample.centers(d.long()).tolist() == [[1.0, 2.0, 3.5, 5.5], [0.5, 1.5, 6.5, 15.5]]
    f = d.double().requires_grad_(True)
    upsample.centers(f, torch.tensor([4, 2])).sum().backward()
    # c_t = sum_{u <= t} d_u - d_t / 2: d_u reaches the centres t >= u, its own by half
    assert f.grad.tolist() == [[3.5, 2.5, 1.5, 0.5], [1.5, 0.5, 0.0, 0.0]]
    for bad in (torch.zeros(3), torch.zeros(2, 3, dtype=torch.bool)):
        with pytest.raises(ValueError, match="centers"):
            upsample.centers(bad)


def test_ops_refuse_before_the_c_call(lib):
    """ValueError for what the header refuses, raised on CPU tensors before anything touches a GPU."""
    import torch
    from tt2 import ops, upsample
    i32 = torch.int32
    h, y, dy = torch.zeros(2, 5, 8), torch.zeros(2, 7, 8), torch.zeros(2, 7, 8)
    c, pr, lse = torch.zeros(2, 5), torch.zeros(2, 5), torch.zeros(2, 7)
    good = dict(h=h, center=c, prec=pr, y=y, lse=lse)
    bad_fwd = [dict(h=h.half(), y=y.half()), dict(h=h.bfloat16()), dict(y=torch.zeros(2, 7, 9)), dict(y=torch.zeros(3, 7, 8)),
               dict(h=h[0]), dict(y=y.transpose(1, 2)), dict(h=torch.zeros(2, 4097, 8), center=torch.zeros(2, 4097), prec=torch.zeros(2, 4097)),
               dict(h=torch.zeros(2, 5, 513), y=torch.zeros(2, 7, 513)), dict(y=torch.zeros(1, 7, 8).expand(2, 7, 8)),
               dict(center=c[:, :4]), dict(center=c.double()), dict(prec=torch.zeros(2, 6)[:, :5]), dict(bias=torch.zeros(2, 4)),
               dict(lse=lse[:, :6]), dict(lse=None), dict(center=None), dict(q_len=torch.zeros(2, dtype=torch.int64)),
               dict(key_len=torch.zeros(3, dtype=i32)), dict(offset=-1.0), dict(offset=float("nan")), dict(offset=float("inf")),
               dict()]                                                    # the last: well-formed, but not on a GPU
    for kw in bad_fwd:
        with pytest.raises(ValueError, match="gauss_upsample_fwd"):
            ops.gauss_upsample_fwd(**{**good, **kw})
    good = dict(good, dy=dy, dh=torch.zeros(2, 5, 8), dcenter=torch.zeros(2, 5), dprec=torch.zeros(2, 5), dbias=torch.zeros(2, 5))
    bad_bwd = [dict(dh=None, dcenter=None, dprec=None, dbias=None), dict(dy=None), dict(dy=torch.zeros(2, 6, 8)), dict(dy=dy.bfloat16()),
               dict(dh=torch.zeros(2, 5, 4)), dict(dh=torch.zeros(2, 4, 8)), dict(dcenter=torch.zeros(2, 4)),
               dict(dprec=torch.zeros(2, 6)[:, :5]), dict(dbias=torch.zeros(2, 5, dtype=torch.float64)), dict(offset=-0.5), dict()]
    for kw in bad_bwd:
        with pytest.raises(ValueError, match="gauss_upsample_bwd"):
            ops.gauss_upsample_bwd(**{**good, **kw})
    d = torch.ones(2, 5, dtype=i32)
    for args, kw in [((h, d), {}),                                        # not on a GPU
                     ((h.double(), d), {}), ((h[0, 0], d), {}), ((h, d[:, :4]), {}), ((h, torch.ones(2, 5, dtype=torch.bool)), {})]:
        with pytest.raises(ValueError, match="gaussian_upsample"):
            upsample.gaussian_upsample(*args, **kw)


def test_host_refusals_and_zero_sizes(lib):
    """Requests refused with TT2_E_INVALID before any launch (there is no GPU here: a launch would
    fail otherwise than with E_INVALID), and the zero-size calls return TT2_OK without one."""
    L = lib.load()
    buf = (ctypes.c_char * 4096)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    E = lib.E_INVALID
    big = 2 ** 31 - 1
    fns = {name: getattr(L, name) for name in ENTRIES}

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

    a = lib.GaussUpsampleArgs()
    for f in ("h", "center", "prec", "bias", "q_len", "key_len", "y", "lse", "dy", "dh", "dcenter", "dprec", "dbias", "workspace"):
        setattr(a, f, ptr)
    a.workspace_bytes = L.tt2_gauss_upsample_bwd_workspace_size(2, 128, 800, 512)
    a.h_ld, a.h_bs, a.y_ld, a.y_bs = 512, 128 * 512, 520, 800 * 520
    a.dy_ld, a.dy_bs, a.dh_ld, a.dh_bs, a.p_ld, a.lse_ld = 520, 800 * 520, 512, 128 * 512, 130, 800
    a.batch, a.tx, a.n_out, a.dim, a.dtype, a.offset = 2, 128, 800, 512, lib.DT_BF16, 0.5
    common = [dict(batch=-1), dict(tx=-1), dict(n_out=-1), dict(dim=-1), dict(tx=4097, p_ld=4097), dict(dim=513, h_ld=513),
              dict(h_ld=511), dict(y_ld=511), dict(h_ld=-1), dict(p_ld=127), dict(lse_ld=799), dict(dtype=lib.DT_F16), dict(dtype=3),
              dict(dtype=-1), dict(offset=-0.25), dict(offset=float("nan")), dict(offset=float("inf")), dict(center=None),
              dict(prec=None), dict(h=None), dict(lse=None), dict(y=None),
              dict(batch=0, dim=-1), dict(batch=0, dtype=2), dict(batch=0, h_ld=1), dict(batch=0, offset=-1.0)]
    none_in = dict(h=None, center=None, prec=None, bias=None, q_len=None, key_len=None)
    check("tt2_gauss_upsample_fwd", a,
          common + [dict(n_out=0, lse_ld=-1), dict(batch=big, n_out=65),          # 2 frame tiles x 4 column chunks
                    dict(batch=big // 4 + 1, n_out=1), dict(n_out=0, dim=513)],
          [dict(batch=0), dict(n_out=0), dict(batch=0, **none_in, y=None, lse=None), dict(n_out=0, **none_in, y=None, lse=None),
           dict(batch=0, tx=4096, p_ld=4096), dict(batch=big // 4, n_out=0), dict(batch=0, dtype=lib.DT_F32)])
    outs_none = dict(dh=None, dcenter=None, dprec=None, dbias=None)
    check("tt2_gauss_upsample_bwd", a,
          common + [dict(dy_ld=511), dict(dh_ld=511), dict(dy=None), dict(workspace=None), dict(workspace_bytes=16),
                    dict(workspace=ptr + 4), outs_none, dict(batch=big, tx=33), dict(batch=big, n_out=5), dict(tx=0, p_ld=-1),
                    dict(n_out=0, **outs_none)],
          [dict(batch=0), dict(tx=0), dict(batch=0, **none_in, **outs_none, y=None, lse=None, dy=None, workspace=None, workspace_bytes=0),
           dict(tx=0, **none_in, **outs_none, y=None, lse=None, dy=None), dict(batch=0, tx=4096, p_ld=4096), dict(batch=big, tx=0, n_out=0),
           dict(batch=0, n_out=0, workspace=None, workspace_bytes=0)])


def test_upsample_struct_layout_matches_c(lib, tmp_path):
    """Every field's offset and the struct's size, from a tiny host program."""
    name, cls = "tt2_gauss_upsample_args", lib.GaussUpsampleArgs
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"tt2_capi.h\"\nint main(){\n"
    prog += f'printf("{name} size %zu\\n", sizeof({name}));\n'
    for field, _ in cls._fields_:
        prog += f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n'
    prog += 'printf("max_dim value %d\\n", TT2_UPSAMPLE_MAX_DIM);\n'
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
        who, field, val = line.split()
        if who == "max_dim":
            assert int(val) == lib.UPSAMPLE_MAX_DIM
        elif field == "size":
            assert ctypes.sizeof(cls) == int(val)
        else:
            assert getattr(cls, field).offset == int(val), field
        seen += 1
    assert seen == 2 + len(cls._fields_)
