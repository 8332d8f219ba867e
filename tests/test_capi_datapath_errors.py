"""CPU: the refusals the data-path entry points share (tt2_invalid and tt2_need_workspace of
csrc/runtime.cpp), pinned to the byte: one "who: message" refusal of each family whose unit had a
formatting helper of its own (forward-sum, attention, DTW, trim, YIN, length regulator, pitch
tracking, resampling, loudness), the workspace refusal of the five entry points that take a
workspace with an alignment (too small, misaligned, null), and the workspace size queries of the two
best-path families at the thresholds where the move bits leave LDS (csrc/align_walk.h).
test_capi_norm_misc.py's pattern: _lib.load(), no device, no launch: every call here returns before
the entry point's first device call.  Written against the library before the helpers were shared
and passing on it unchanged."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import os
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


@pytest.fixture(scope="module")
def mem():
    """Host memory the refused calls may point at (never read); the address is 64-B aligned."""
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 63) & ~63


def _refused(lib, L, call, text):
    """call() returns TT2_E_INVALID and leaves exactly `text`; an unrelated refusal first, so that
    the message read afterwards belongs to the call under test."""
    assert L.tt2_version() == 1
    assert L.tt2_regulate_fwd(None, None) == lib.E_INVALID
    assert L.tt2_last_error() == b"tt2_regulate_fwd: args required"
    assert call() == lib.E_INVALID
    assert L.tt2_last_error() == text.encode(), (text, L.tt2_last_error())


def test_e_invalid_value(lib):
    assert lib.E_INVALID == -1


@pytest.mark.parametrize("entry", ["tt2_forward_sum_fwd", "tt2_forward_sum_bwd", "tt2_forward_sum_path",
                                   "tt2_align_monotonic", "tt2_attn_align", "tt2_align_durations", "tt2_dtw",
                                   "tt2_trim", "tt2_yin", "tt2_regulate_plan", "tt2_regulate_bwd", "tt2_pitch_track",
                                   "tt2_resample", "tt2_loudness"])
def test_null_args(lib, entry):
    L = lib.load()
    _refused(lib, L, lambda: getattr(L, entry)(None, None), entry + ": args required")


def test_a_negative_size_per_family(lib, mem):
    L = lib.load()
    _, p = mem
    cases = [
        ("tt2_forward_sum_path", lib.ForwardSumArgs(batch=1, tq=-1, tk=1), "negative batch / tq / tk"),
        ("tt2_align_monotonic", lib.AlignMonoArgs(head_dim=64, n_layers=1, dtype=lib.DT_BF16, batch=-1, heads=1, scale=1.0),
         "shape / scale"),
        ("tt2_attn_align", lib.AlignArgs(head_dim=32), "head_dim must be 64"),
        ("tt2_dtw", lib.DtwArgs(batch=1, ta=1, tb=-1), "negative batch / ta / tb"),
        ("tt2_trim", lib.TrimArgs(hop=1, r=1, keep=0, ratio=0.5, batch=-1), "negative batch / n_in / n_out"),
        ("tt2_yin", lib.YinArgs(tau_min=1, tau_max=2, hop=1, t=-1), "hop < 1 or negative utt_stride / batch / t"),
        ("tt2_regulate_plan", lib.RegulatePlanArgs(batch=1, tx=1, n_out=-1), "negative batch / tx / n_out"),
        ("tt2_regulate_fwd", lib.RegulateArgs(batch=1, tx=1, n_out=1, dim=-1), "negative batch / tx / n_out / dim"),
        ("tt2_pitch_track", lib.PitchTrackArgs(tau_min=1, tau_max=2, batch=-1), "negative batch / t"),
        ("tt2_resample", lib.ResampleArgs(up=1, down=1, half=1, n_in=-1), "negative batch / n_in / n_out"),
        ("tt2_loudness", lib.LoudnessArgs(step=1, n_out=-1), "negative batch / n_in / n_out"),
    ]
    for entry, a, msg in cases:
        _refused(lib, L, lambda: getattr(L, entry)(ctypes.byref(a), None), f"{entry}: {msg}")


def _dtw(lib, p):
    a = lib.DtwArgs(batch=2, ta=40, tb=30, c0=0, c1=4, a_ld=4, b_ld=4)
    a.a = a.b = a.total = a.length = a.path_a = a.path_b = p
    return a, lib.load().tt2_dtw_workspace_size(2, 40, 30, 1)


def _pitch_track(lib, p):
    a = lib.PitchTrackArgs(batch=2, t=8, tau_min=2, tau_max=10, cmnd_ld=11, sr=16000.0, jump=0.1, switch_cost=0.1,
                           unvoiced=0.1)
    a.cmnd = a.pos = a.f0 = a.lag = a.cost = p
    return a, lib.load().tt2_pitch_track_workspace_size(2, 8, 2, 10)


def _fsum(lib, p, tq, tk):
    a = lib.ForwardSumArgs(batch=2, tq=tq, tk=tk, s_ld=tk, s_bs=tq * tk, a_ld=tk, d_ld=tk, d_bs=tq * tk)
    a.scores = a.lse = a.alpha = a.dscores = a.path = a.durations = a.logp = p
    return a


def _fsum_bwd(lib, p):
    return _fsum(lib, p, 8, 5), lib.load().tt2_forward_sum_bwd_workspace_size(2, 8, 5)


def _fsum_path(lib, p):
    return _fsum(lib, p, 300, 260), lib.load().tt2_forward_sum_path_workspace_size(2, 300, 260)


def _mono(lib, p):
    a = lib.AlignMonoArgs(n_layers=1, batch=2, heads=2, head_dim=64, tq=300, tk=260, dtype=lib.DT_BF16, q_ld=128,
                          k_ld=128, scale=0.125)
    a.q[0] = a.k[0] = a.lse[0] = p
    a.path = a.durations = a.logp = p
    return a, lib.load().tt2_align_monotonic_workspace_size(2, 300, 260)


# entry point, its request with everything but the workspace in order, the alignment it asks for
WORKSPACE = [("tt2_dtw", _dtw, 4), ("tt2_pitch_track", _pitch_track, 4), ("tt2_forward_sum_bwd", _fsum_bwd, 16),
             ("tt2_forward_sum_path", _fsum_path, 8), ("tt2_align_monotonic", _mono, 8)]


@pytest.mark.parametrize("entry,make,align", WORKSPACE, ids=[w[0] for w in WORKSPACE])
def test_workspace_refusals(lib, mem, entry, make, align):
    L = lib.load()
    _, p = mem
    a, need = make(lib, p)
    assert need > 0
    text = f"{entry}: workspace too small or misaligned: {need} bytes needed"
    for ws, have in ((p, need - 1), (p + align // 2, need), (None, need)):
        a.workspace, a.workspace_bytes = ws, have
        _refused(lib, L, lambda: getattr(L, entry)(ctypes.byref(a), None), text)


def test_needed_sizes(lib):
    L = lib.load()
    assert L.tt2_dtw_workspace_size(2, 40, 30, 1) == 2 * ((40 + 15) // 16) * 30 * 4   # a move word per 16 rows
    assert L.tt2_pitch_track_workspace_size(2, 8, 2, 10) == 2 * 8 * 10 * 4
    assert L.tt2_forward_sum_bwd_workspace_size(2, 8, 5) == 2 * 8 * 128 * 4
    assert L.tt2_forward_sum_bwd_workspace_size(2, 8, 129) == 2 * 8 * 256 * 4
    assert L.tt2_forward_sum_bwd_workspace_size(2, 8, 257) == 2 * 8 * 512 * 4


@pytest.mark.parametrize("query", ["tt2_align_monotonic_workspace_size", "tt2_forward_sum_path_workspace_size"])
def test_move_bits_leave_lds_at_the_same_lengths(lib, query):
    """8 bytes per 64 keys of capacity (128, 256 or 512) and frame; the kernels keep 65536, 49152
    and 16384 bytes of LDS for them, so the workspace begins above 4096 (never: the largest tq),
    1536 and 256 frames."""
    size = getattr(lib.load(), query)
    for tk in (1, 64, 128):
        assert size(3, 4096, tk) == 0
    for tk in (129, 200, 256):
        assert size(3, 1536, tk) == 0
        assert size(3, 1537, tk) == 3 * 1537 * 4 * 8
        assert size(1, 4096, tk) == 4096 * 4 * 8
    for tk in (257, 300, 512):
        assert size(3, 256, tk) == 0
        assert size(3, 257, tk) == 3 * 257 * 8 * 8
        assert size(1, 4096, tk) == 4096 * 8 * 8
    for args in ((0, 300, 300), (-1, 300, 300), (1, 0, 300), (1, 300, 0), (1, 300, 513)):
        assert size(*args) == 0
