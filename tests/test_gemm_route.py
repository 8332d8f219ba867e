"""The GEMM host routing, pinned request by request (host logic, CPU): tt2_gemm_plan and
tt2_gemm_stats_rows replayed over a sweep of sizes, layouts, splits, forced variants, epilogue
options, C alignment and output dtype against tests/golden/gemm_route.npz.

The fixture records what the library answered BEFORE the planner / dispatcher was reorganised
into one route function; it is never regenerated from the code under test.  To record it from
another build of the library (an older commit's):
    TT2_LIB=/path/to/older/libtt2.so python tests/test_gemm_route.py --write
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "transformer-tacotron2_amd"))
from tt2 import _lib  # noqa: E402
from tt2._lib import ACT_TANH, DT_BF16, DT_F32  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_route.npz")

MS = (64, 256, 2048, 12800)
NS = (80, 128, 512, 576, 1536, 2048)
KS = (64, 512, 2048, 6144)
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
SPLITS = (1, 2)
VARIANTS = (0, 1, 2, 3, 13, 14, 15, 16, 17)
OPTIONS = ("none", "bias", "res", "gate", "tanh", "beta", "conv_a")
C_OFFSETS = (0, 8)           # C pointer: 16-B aligned, or 8 bytes past it
DTYPES_OUT = (DT_BF16, DT_F32)

# the plan reads sizes, flags and pointer alignment only: the pointers are never followed
_P_OPER, _P_C, _P_BIAS, _P_X = 0x100000, 0x200000, 0x300000, 0x400000


def sweep(lib):
    """(plan, stats_rows) int16 arrays over the whole sweep, in itertools.product order."""
    plan_f, rows_f = lib.tt2_gemm_plan, lib.tt2_gemm_stats_rows
    plan_f.argtypes = rows_f.argtypes = [C.POINTER(_lib.GemmArgs)]
    plan_f.restype, rows_f.restype = C.c_int, C.c_int32
    plans, rows = [], []
    for m, n, k, (ta, tb), sp, var in itertools.product(MS, NS, KS, LAYOUTS, SPLITS, VARIANTS):
        for opt in OPTIONS:
            g = _lib.GemmArgs()
            g.a = g.b = _P_OPER
            g.m, g.n, g.k = m, n, k
            g.lda, g.ldb, g.ldc = (m if ta else k), (n if tb else k), n
            g.dtype_in = DT_BF16
            g.trans_a, g.trans_b = ta, tb
            g.alpha, g.gate_scale = 1.0, 1.0
            g.splits, g.kernel_variant = sp, var
            if opt == "bias":
                g.bias = _P_BIAS
            elif opt == "res":
                g.res, g.ldr, g.res_dtype = _P_X, n, DT_BF16
            elif opt == "gate":
                g.gate, g.ldg, g.gate_dtype = _P_X, n, DT_BF16
            elif opt == "tanh":
                g.act = ACT_TANH
            elif opt == "beta":
                g.beta = 1.0
            elif opt == "conv_a":   # 64 frames x 64 channels per tap
                g.a_conv_t, g.a_conv_c, g.a_conv_pad, g.lda = 64, 64, 2, 64
            ref = C.byref(g)
            for off, dt in itertools.product(C_OFFSETS, DTYPES_OUT):
                g.c, g.dtype_out = _P_C + off, dt
                plans.append(plan_f(ref))
                rows.append(rows_f(ref))
    return np.asarray(plans, np.int16), np.asarray(rows, np.int16)


def test_plan_and_stats_rows_match_the_recorded_routing():
    want = np.load(GOLDEN)
    plans, rows = sweep(C.CDLL(_lib.LIB_PATH))   # host code: no HIP device needed
    assert plans.shape == want["plan"].shape and plans.size > 100000
    bad = np.flatnonzero((plans != want["plan"]) | (rows != want["stats_rows"]))
    assert bad.size == 0, (f"{bad.size} requests route differently; first at sweep index {bad[0]}: plan "
                           f"{plans[bad[0]]} (recorded {want['plan'][bad[0]]}), stats rows {rows[bad[0]]} "
                           f"(recorded {want['stats_rows'][bad[0]]})")
    # the sweep reaches every kernel family and both chunk heights
    assert set(np.unique(want["plan"])) == {1, 2, 3, 13, 15, 16, 17}
    assert set(np.unique(want["stats_rows"])) == {0, 64, 256}


def _refused(**fields):
    """tt2_gemm on a request that is refused before any launch (host code): the error text"""
    lib = C.CDLL(_lib.LIB_PATH)
    lib.tt2_gemm.argtypes, lib.tt2_gemm.restype = [C.POINTER(_lib.GemmArgs), C.c_void_p], C.c_int
    lib.tt2_last_error.restype = C.c_char_p
    g = _lib.GemmArgs()
    g.a = g.b = _P_OPER
    g.c, g.col_stats = _P_C, _P_X
    g.m, g.n, g.k = 32, 128, 512
    g.lda = g.ldb = 512
    g.ldc = 128
    g.dtype_in = g.dtype_out = DT_BF16
    g.alpha = 1.0
    for k, v in fields.items():
        setattr(g, k, v)
    assert lib.tt2_gemm(C.byref(g), None) != 0
    return lib.tt2_last_error().decode()


def test_statistics_on_a_skinny_request_report_the_statistics_error():
    """A fused-statistics request whose plan is the skinny path: the forced-v7 plan it would need
    fails on its own (f16 operands, a decode fusion), and the error stays the one about the
    statistics, as before the route function."""
    want = "tt2_gemm: col_stats / bn_bwd need the v8 path or v7's LDS-image path"
    assert _refused(dtype_in=_lib.DT_F16).startswith(want)
    assert _refused(pe_table=_P_X, pe_alpha=_P_X, pe_t=_P_X).startswith(want)
    # the planner's own refusals keep their text
    assert _refused(dtype_in=_lib.DT_F16, m=128).startswith("tt2_gemm: f16 operands only on the skinny decode path")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        raise SystemExit(__doc__)
    p, r = sweep(C.CDLL(_lib.LIB_PATH))
    np.savez_compressed(GOLDEN, plan=p, stats_rows=r)
    print(GOLDEN, p.size, "requests; plans", np.unique(p), "rows", np.unique(r))
