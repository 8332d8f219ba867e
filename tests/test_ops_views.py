"""CPU: the view and vector validators of the data-path wrappers in tt2.ops (dtw .. regulate_*), called
directly on host tensors, and the refusals of resample / trim / loudness / regulate_plan that are built
from them.  Every refusal fires before the library is loaded, so nothing here needs a GPU."""
import pytest
import torch

from tt2 import ops
from tt2._lib import TT2Error

f32, i32 = torch.float32, torch.int32


def strided(rows, cols, stride, dtype=f32):
    return torch.zeros(64, dtype=dtype).as_strided((rows, cols), (stride, 1))


def test_leading_dimension_of_row_views():
    assert ops._rows("op", "t", torch.zeros(4, 10)[:, :7], f32) == 10
    assert ops._rows("op", "t", torch.zeros(4, 10), f32, rows=4, min_cols=10) == 10
    # a single row's stride is arbitrary: any value that covers the row
    assert ops._rows("op", "t", strided(1, 7, 0), f32) == 7
    assert ops._rows("op", "t", strided(1, 7, 3), f32) == 7
    assert ops._rows("op", "t", strided(1, 7, 9), f32) == 9
    assert ops._rows("op", "t", strided(2, 7, 7), f32) == 7
    # nothing to overlap: zero columns, zero rows
    assert ops._rows("op", "t", torch.zeros(3, 0), f32) >= 0
    assert ops._rows("op", "t", torch.zeros(0, 5), f32) == 5
    assert ops._rows("op", "t", torch.zeros(2, 5, dtype=i32), i32, rows=2, min_cols=5, err=ValueError) == 5


@pytest.mark.parametrize("err", [TT2Error, ValueError])
def test_row_views_refused(err):
    bad = [(strided(2, 7, 3), {}, "overlap"),                      # two rows three elements apart
           (torch.zeros(7, 4).t(), {}, "contiguous last dim"),     # transposed: the last dim strides
           (torch.zeros(4, 7, dtype=torch.float64), {}, "float32"),
           (torch.zeros(4, 7, dtype=i32), {}, "float32"),
           (torch.zeros(7), {}, "contiguous last dim"), (torch.zeros(2, 4, 7), {}, "contiguous last dim"),
           (torch.zeros(4, 7), dict(rows=3), "3"), (torch.zeros(4, 7), dict(min_cols=8), "8")]
    for t, kw, word in bad:
        with pytest.raises(err, match="op: arg") as e:
            ops._rows("op", "arg", t, f32, err=err, **kw)
        assert word in str(e.value), (word, str(e.value))
        assert type(e.value) is err


def test_vectors_exact_and_at_least():
    B = 4
    good = torch.zeros(B, dtype=i32)
    for exact in (False, True):
        ops._vec("op", "v", good, B, i32, exact=exact)
        ops._vec("op", "v", None, B, i32, exact=exact)                     # optional arguments pass through
        for bad in (torch.zeros(B - 1, dtype=i32), torch.zeros(B), torch.zeros(B, dtype=torch.int64),
                    torch.zeros(2 * B, dtype=i32)[::2]):
            with pytest.raises(TT2Error, match="op: v"):
                ops._vec("op", "v", bad, B, i32, exact=exact)
    # at least numel elements of any shape, or exactly [B]
    for roomy in (torch.zeros(2, B, dtype=i32), torch.zeros(B + 3, dtype=i32)):
        ops._vec("op", "v", roomy, B, i32)
        with pytest.raises(ValueError, match="op: v"):
            ops._vec("op", "v", roomy, B, i32, exact=True, err=ValueError)


def test_same_gpu_refuses_host_tensors_and_skips_none():
    ops._same_gpu("op", (None, None))
    for tensors, err in (((torch.zeros(2), None), TT2Error), ((None, torch.zeros(2), torch.zeros(2)), ValueError)):
        with pytest.raises(err, match="op: every tensor"):
            ops._same_gpu("op", tensors, err=err)


def test_workspace_binding_leaves_a_zero_need_alone():
    class Args:
        workspace, workspace_bytes = None, 0
    g = Args()
    ops._bind_workspace(g, 0, None)                    # no bytes needed: no allocation, nothing set
    assert (g.workspace, g.workspace_bytes) == (None, 0)


X, Y, LENS = torch.zeros(2, 64), torch.zeros(2, 64), torch.zeros(2, dtype=i32)
COEF = (1.0, 0.0, 0.0, 0.0, 0.0) * 2
WRAPPERS = {
    "resample": lambda **kw: ops.resample(kw.get("x", X), kw.get("y", Y), torch.zeros(1, 3), 1, 2, 1, lens=kw.get("lens")),
    "trim": lambda **kw: ops.trim(kw.get("x", X), kw.get("y", Y), 8, 2, 0, 0.001, lens=kw.get("lens")),
    "loudness": lambda **kw: ops.loudness(kw.get("x", X), 16, COEF, 0.0, 0.1, 0.01, 0.9, lens=kw.get("lens"),
                                          y=kw.get("y", Y)),
}


@pytest.mark.parametrize("op", sorted(WRAPPERS))
def test_wrappers_refuse_overlapping_rows_and_float_lens(op):
    call = WRAPPERS[op]
    with pytest.raises(TT2Error, match=f"{op}: y.*overlap"):
        call(y=strided(2, 7, 3))
    with pytest.raises(TT2Error, match=f"{op}: x"):
        call(x=torch.zeros(64, 2).t())
    with pytest.raises(TT2Error, match=f"{op}: lens"):
        call(lens=LENS.float())
    with pytest.raises(TT2Error, match=f"{op}: lens"):
        call(lens=torch.zeros(4, dtype=i32)[::2])
    with pytest.raises(TT2Error, match=f"{op}: every tensor"):      # well-formed, but not on a GPU
        call(lens=LENS)


def test_regulate_plan_refuses_the_same_faults_with_value_error():
    d = torch.zeros(2, 7, dtype=i32)
    with pytest.raises(ValueError, match="regulate_plan: ends.*overlap"):
        ops.regulate_plan(d, 4, ends=strided(2, 7, 3, i32))
    with pytest.raises(ValueError, match="regulate_plan: durations.*overlap"):
        ops.regulate_plan(strided(2, 7, 3, i32), 4, ends=torch.zeros(2, 7, dtype=i32))
    for name in ("key_len", "frames", "total"):
        with pytest.raises(ValueError, match=f"regulate_plan: {name}"):
            ops.regulate_plan(d, 4, ends=torch.zeros(2, 7, dtype=i32), **{name: torch.zeros(2)})
    with pytest.raises(ValueError, match="regulate_plan: key_len"):  # regulate_* wants exactly [B]
        ops.regulate_plan(d, 4, ends=torch.zeros(2, 7, dtype=i32), key_len=torch.zeros(2, 2, dtype=i32))
