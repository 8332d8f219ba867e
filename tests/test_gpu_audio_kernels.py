"""Every kernel of csrc/audio.hip on its own, through the C ABI (tt2._lib), against the float64
references of tests/_audio_refs.py (pinned to the oracle and shown to bite, with mutants, by
tests/test_audio_refs.py), and the state the pipeline of tt2/audio.py keeps between calls.

  * Moves and exact-arithmetic problems (reflect padding, Pythagorean magnitudes, phases on the
    axes, one-hot overlap-add cells, integer grids) are held bit for bit.
  * The other problems are held per element to float64: the two derived ulp bars of the magnitude
    (2 ulp) and the rephase (3 ulp), the project's yardstick max(4 x the error of the float32 twin
    on the CPU, 2 ulp) (_misc_refs.worst_ratio <= 1) for the overlap-add, log and exp, and the GEMM
    yardstick (_gemm_refs.judge_random) for the STFT stage.  Each test prints its worst ratio
    (pytest -s).
  * Every output is NaN-filled inside guards (before, after, and the columns between the logical
    width and the leading dimension where the kernel does not own them); the guards must still be
    NaN afterwards and no NaN may be left inside.  Every input the contract says is not read is
    NaN: rows at and beyond an utterance's frame count (the rows that straddle two utterances among
    them), samples at and beyond lens[b], the columns between the logical width and the leading
    dimension.
  * One case per kernel has just over 16384 x 256 elements, so that the second trip of its
    grid-stride loop runs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _audio_refs as A  # noqa: E402
import _gemm_refs as G  # noqa: E402
from tt2 import _lib  # noqa: E402
from tt2.audio import HOP, LD_MAG, LD_SPEC, N_FFT, N_MELS, NB, GriffinLim, MelExtractor  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 8


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Out:
    """A NaN-filled f32 buffer of GUARD + rows * ld + GUARD elements; the kernel gets the middle as
    [rows, ld] and owns its first `cols` columns."""

    def __init__(self, rows, cols, ld):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.flat = torch.full((2 * GUARD + rows * ld,), NAN, dtype=torch.float32, device=DEV)

    def ptr(self):
        return self.flat.data_ptr() + 4 * GUARD

    def untouched(self):
        return bool(torch.isnan(self.flat).all().item())

    def collect(self, what):
        """The logical [rows, cols] part as numpy, after the guard checks."""
        f = self.flat.cpu()
        assert torch.isnan(f[:GUARD]).all() and torch.isnan(f[-GUARD:]).all(), f"{what}: guard before / after written"
        body = f[GUARD:-GUARD].view(self.rows, self.ld)
        assert torch.isnan(body[:, self.cols:]).all(), f"{what}: guard columns written"
        assert not torch.isnan(body[:, :self.cols]).any(), f"{what}: NaN left inside the logical extent"
        return body[:, :self.cols].contiguous().numpy()


def call(name, *args):
    return getattr(_lib.lib(), name)(*args, _lib.stream_ptr())


def ok(name, *args):
    _lib.check(call(name, *args), name)


# ------------------------------------------------------------------ one launch per kernel
def run_reflect_pad(p):
    x, lens = dev(p["x"]), dev(p["lens"])
    out = Out(p["batch"], p["padded_len"], p["padded_len"])
    ok("tt2_reflect_pad", x.data_ptr(), p["ldx"], _lib.ptr(lens), p["batch"], p["len"], out.ptr(), p["padded_len"],
       p["pad"])
    return out.collect(p["name"])


def run_spec_magnitude(p):
    spec = dev(p["spec"])
    out = Out(p["m"], p["ld_mag"], p["ld_mag"])
    ok("tt2_spec_magnitude", spec.data_ptr(), p["ld_spec"], p["m"], p["n_bins"], out.ptr(), p["ld_mag"])
    return out.collect(p["name"])


def run_spec_rephase(p):
    mag, est = dev(p["mag"]), dev(p["est"])
    out = Out(p["m"], p["ld_out"], p["ld_out"])
    ok("tt2_spec_rephase", mag.data_ptr(), p["ld_mag"], _lib.ptr(est), p["ld_est"], p["m"], p["n_bins"], out.ptr(),
       p["ld_out"])
    return out.collect(p["name"])


def run_overlap_add(p, ld_y=None):
    ld_y = ld_y or p["len"]
    frames, lens = dev(p["frames"]), dev(p["lens"])
    out = Out(p["batch"], p["len"], ld_y)
    ok("tt2_overlap_add", frames.data_ptr(), p["ld_frames"], _lib.ptr(lens), p["batch"], p["len"], p["rows_per_utt"],
       p["n_fft"], p["hop"], out.ptr(), ld_y)
    return out.collect(p["name"])


def run_mel_gather(p):
    rows, frames = dev(p["rows"]), dev(p["frames"])
    B, T, C = p["batch"], p["t"], p["n_mels"]
    out = Out(B * T, C, C)
    ok("tt2_mel_rows", rows.data_ptr(), p["ld_rows"], out.ptr(), _lib.ptr(frames), B, T, C, p["rows_per_utt"],
       p["clamp"], 0)
    return out.collect(p["name"]).reshape(B, T, C)


def run_mel_scatter(p):
    mel, frames = dev(p["mel"]), dev(p["frames"])
    B, T, C = p["batch"], p["t"], p["n_mels"]
    out = Out(B * p["rows_per_utt"], C, p["ld_rows"])
    ok("tt2_mel_rows", out.ptr(), p["ld_rows"], mel.data_ptr(), _lib.ptr(frames), B, T, C, p["rows_per_utt"],
       p["clamp"], 1)
    return out.collect(p["name"])


RUN = {"reflect_pad": run_reflect_pad, "spec_magnitude": run_spec_magnitude, "spec_rephase": run_spec_rephase,
       "overlap_add": run_overlap_add, "mel_gather": run_mel_gather, "mel_scatter": run_mel_scatter}


def hold(p, got=None):
    """Run problem p (unless its output is given), judge it, print the verdict, assert."""
    got = RUN[p["kernel"]](p) if got is None else got
    good, text = A.judge(p, got)
    print(f"\n{p['kernel']} {p['name']}: {text}", end="")
    assert good, f"{p['kernel']} {p['name']}: {text}"
    return got


# ------------------------------------------------------------------ the kernels
def test_reflect_pad():
    """Bit-exact (a move of samples that are each their own integer).  (pad, len, padded_len) =
    (4, 9, 24): padded_len larger than len + 2 pad rounded up; (512, 1300, 2560) and (512, 513, 1792):
    exactly that.  One batch holds lens = {len, len - 1, pad + 1, pad, 1, 0, -3, len + 7}: np.pad's
    reflection, the clamp rule of lens[b] <= pad, zero rows, and an entry above len; once with
    ldx = len and once with ldx = len + 5 and NaN between the utterances; lens = NULL.  Samples at and
    beyond lens[b] are NaN."""
    for p in A.reflect_pad_problems():
        got = hold(p)
        for b in range(p["batch"]):
            n = max(0, A.eff_len(p["lens"], b, p["len"]))
            assert not got[b, (n + 2 * p["pad"] if n else 0):].any(), (p["name"], b)


@pytest.mark.parametrize("nb", [1, 5, 513])
def test_spec_magnitude(nb):
    """ld_mag in {n_bins, n_bins + 3} x ld_spec in {2 n_bins, 2 n_bins + 6} (the extra columns NaN).
    selector: Pythagorean integer pairs and (x, 0) / (0, x) times powers of two, every sign: re^2 +
    im^2 is a perfect square below 2^24 units, so the result is exact.
    random: |re|, |im| from 2^-40 to 2^40, each result within 2 f32 ulp of the float64 value of the
    f32 inputs.  Derivation, in units of the result r = sqrt(s), s = re^2 + im^2: the two products
    (or one product and one fma) and the add each round by at most half an ulp of a value no larger
    than s, so the computed s is off by at most 1.25 ulp(s) (the products' ulps sum to at most 3/2
    of ulp(s)/2 when one is a binade below); the square root halves the relative error, which in
    ulp(r) is at most 0.625 sqrt(m) / m for s = 4^k m with m in [1, 2) and 1.25 / sqrt(m) for m in
    [2, 4), that is below 0.89; the correctly rounded sqrtf adds 0.5: under 1.4 ulp.  sqrtf and / are
    correctly rounded in this build: hipcc's -fhip-fp32-correctly-rounded-divide-sqrt is on by
    default and build_lib.py passes neither -fno-hip-fp32-correctly-rounded-divide-sqrt nor
    -ffast-math; the exact selector problem would fail otherwise.
    The padding columns [n_bins, ld_mag) are +0 (bit-exact problems compare them; the random ones
    check them here)."""
    problems = [p for p in A.magnitude_problems() if p["n_bins"] == nb]
    assert len(problems) == 8
    for p in problems:
        got = hold(p)
        assert not got[:, nb:].view(np.int32).any(), p["name"]


@pytest.mark.parametrize("nb", [7, 513])
def test_spec_rephase(nb):
    """ld_out in {2 n_bins, 2 n_bins + 6, 3 n_bins}, ld_mag and ld_est with and without extra (NaN)
    columns.  Bit-exact: est = NULL gives re = mag and im = +0; est on an axis, (+-x, 0) or
    (0, +-x), gives exactly +-mag (sqrtf(x * x) == |x| and x / |x| == +-1 under correct rounding);
    e == 0 gives phase 0.
    random: each component within 3 f32 ulp of the float64 value of the f32 inputs, and re^2 + im^2
    within the same bar of mag^2 (|re^2 + im^2 - mag^2| <= 2 mag x 3 ulp(mag)).  Derivation, each
    correctly rounded operation adding at most half an ulp of its own result: |e| as in
    test_spec_magnitude (under 1.4 ulp), the division 0.5, the product with mag 0.5: 2.4 ulp when the
    operands' mantissas are alike.  (In relative terms the chain is (1 + u)^4 with u = 2^-24, which
    is 2 to 4 ulp of the result depending on its mantissa; the errors would all have to align to
    pass 3, and the printed ratio shows how far the kernel stays from it.)  The flag that makes
    sqrtf and / correctly rounded is named in test_spec_magnitude.
    The padding columns [2 n_bins, ld_out) are +0 and nothing is written beyond ld_out."""
    problems = [p for p in A.rephase_problems() if p["n_bins"] == nb]
    assert len(problems) == 18
    for p in problems:
        got = hold(p)
        assert not got[:, 2 * nb:].view(np.int32).any(), p["name"]
        if p["est"] is None:
            assert A.bits_equal(got[:, :nb], p["mag"][:, :nb]) and not got[:, nb:].view(np.int32).any(), p["name"]


@pytest.mark.parametrize("n_fft,hop", A.OLA_GEOMETRIES)
def test_overlap_add_onehot(n_fft, hop):
    """One cell frames[b * R + f][n] = 1, everything else 0: the output is nonzero at exactly the one
    sample t = f hop + n - n_fft / 2 of utterance b (0 there too when t is outside [0, len_b) or the
    divisor is at most 1e-8), every other sample exactly +0, its value within the yardstick of
    1 / sum hann^2.  The cell walks f in {0, 1, nf - 1, nf} (a frame at nf_b must not appear), n in
    {0, 1, hop - 1, hop, n_fft - 1}, the first and the last utterance; ld_y = len + 5 with guards."""
    lens, cells = A.ola_onehot_cells(n_fft, hop)
    worst = 0.0
    for cell in cells:
        p = A.ola_onehot_problem(n_fft, hop, lens, cell)
        got = run_overlap_add(p, p["len"] + 5)
        good, text = A.judge(p, got)
        assert good, f"{p['name']}: {text}"
        worst = max(worst, float(text.split()[1])) if text.startswith("ratio") else worst
        where = A.ola_onehot_expected(p)
        nz = [tuple(i) for i in np.argwhere(got != 0)]
        assert nz == [] if where is None else all(i == where for i in nz), (p["name"], nz, where)
        if where is not None:
            assert (got[where] != 0) == (A.reference(p)[where] != 0), p["name"]
    print(f"\noverlap_add one-hot ({n_fft}, {hop}): {len(cells)} cells, worst ratio {worst:.3f}", end="")


@pytest.mark.parametrize("n_fft,hop", A.OLA_GEOMETRIES)
def test_overlap_add_random(n_fft, hop):
    """Seeded frames against float64 through the float32 twin (window as sin^2(pi n / n_fft) in
    float32), worst_ratio <= 1, with lens = {3 hop, 3 hop - 1, 1, 0, len, len + 5}, ld_y = len and
    len + 5, ld_frames = n_fft + 3; frame rows at and beyond 1 + len_b / hop (the straddle rows among
    them) and the extra columns are NaN.  No compared sample has a float64 divisor within a factor 2
    of the 1e-8 threshold (asserted: nothing is excluded).

    This test decided the window's form.  With the window as 0.5f - 0.5f * cosf(2 pi n / n_fft) the
    device gave the ratios of the first row; the kernel now squares sinf(pi min(n, n_fft - n) / n_fft)
    and gives the second:
        (n_fft, hop)   (1024, 256)  (64, 16)  (64, 32)  (64, 64)  (48, 20)  (9, 4)
        cos form       0.728        0.213     4.581     81.862    1.240     0.384
        sin^2 form     0.250        0.250     0.338     0.250     0.250     0.250"""
    p = A.ola_random_problem(n_fft, hop)
    assert A.ola_borderline(p) == 0
    for ld_y in (p["len"], p["len"] + 5):
        got = hold(p, run_overlap_add(p, ld_y))
        for b in range(p["batch"]):
            assert not got[b, max(0, A.eff_len(p["lens"], b, p["len"])):].view(np.int32).any(), (p["name"], b)


def test_mel_rows():
    """t in {1, rows_per_utt, rows_per_utt - 3} x ld_rows in {n_mels, n_mels + 4} x frames in {NULL, all
    t, {t, t + 3, 1, 0, -2, t - 1}}.
    gather: worst_ratio <= 1 against float64 log through the numpy float32 twin; inputs from 1e-12 to
    1e6 with exactly clamp, the next value above it, +-0, a negative value and 1.0 among them; every
    silence element holds the same bits (and the judge holds them to log(clamp)); rows at
    and beyond frames[b] are NaN (never read).
    scatter: worst_ratio <= 1 for exp over [-12, 6]; every row at t >= frames[b], the rows in
    [t, rows_per_utt) included, is exactly +0 (the judge holds them to those bits); mel rows at and
    beyond frames[b] are NaN; the columns [n_mels, ld_rows) are not written.

    This test found the gather outside its bar: with logf the device gave ratios 0.80 to 1.056 (2.11
    ulp at the worst element, 1.74 ulp at log(clamp), against a float32 twin within 0.54 ulp).  The
    kernel now rounds the double log once and gives 0.21 to 0.25; the scatter's expf gives 0.04 to
    0.25 and is as it was."""
    silence = set()
    for p in A.mel_rows_problems():
        got = hold(p)
        if p["kernel"] == "mel_gather":
            for b in range(p["batch"]):
                silence |= set(got[b, A._nf(p["frames"], b, p["t"]):].view(np.int32).reshape(-1).tolist())
    assert len(silence) == 1, f"silence rows hold {len(silence)} different bit patterns"


GRID = {"reflect_pad": A.reflect_pad_grid_problem, "spec_magnitude": A.magnitude_grid_problem,
        "spec_rephase": A.rephase_grid_problem, "overlap_add": A.ola_grid_problem,
        "mel_gather": lambda: A.mel_rows_grid_problems()[0], "mel_scatter": lambda: A.mel_rows_grid_problems()[1]}


@pytest.mark.parametrize("kernel", list(GRID))
def test_grid_stride_second_trip(kernel):
    """Just over 16384 blocks x 256 threads of elements (the launch's cap), so the loop's second trip
    runs, with integer-valued inputs: the pad, the magnitude (Pythagorean pairs) and the rephase (est
    on the axes) bit-exact; the overlap-add of small integers (n_fft 8, hop 4), the log of {1, below
    clamp} and the exp of {0, -inf} through the yardstick, their zeros bit-exact."""
    p = GRID[kernel]()
    total = {"reflect_pad": lambda: p["batch"] * p["padded_len"], "spec_magnitude": lambda: p["m"] * p["ld_mag"],
             "spec_rephase": lambda: p["m"] * p["n_bins"], "overlap_add": lambda: p["batch"] * p["len"],
             "mel_gather": lambda: p["batch"] * p["rows_per_utt"] * p["n_mels"],
             "mel_scatter": lambda: p["batch"] * p["rows_per_utt"] * p["n_mels"]}[kernel]()
    assert A.GRID_CAP < total < A.GRID_CAP + 2 ** 17
    if kernel == "overlap_add":
        assert A.ola_borderline(p) == 0
    hold(p)


def test_refusals_leave_the_output_untouched():
    """One refusal of each kind the host checks added for this family (and one older one per entry):
    TT2_E_INVALID, and the NaN-filled output is still all NaN."""
    src = torch.ones(4096, device=DEV)
    cnt = torch.ones(8, dtype=torch.int32, device=DEV)
    out = Out(1, 4096, 4096)
    s, c, o = src.data_ptr(), cnt.data_ptr(), out.ptr()
    refused = [("tt2_reflect_pad", (s, 100, c, 2, 100, o, 256, -1)),
               ("tt2_reflect_pad", (s, 99, c, 2, 100, o, 256, 8)),
               ("tt2_reflect_pad", (s, 100, c, 2, 100, o, 115, 8)),
               ("tt2_spec_magnitude", (s, 10, 4, 5, o, 4)),
               ("tt2_spec_rephase", (s, 4, s, 10, 4, 5, o, 10)),
               ("tt2_spec_rephase", (s, 5, s, 10, 4, 5, o, 16)),
               ("tt2_overlap_add", (s, 64, c, 2, 100, 11, 64, 16, o, 99)),
               ("tt2_overlap_add", (s, 64, c, 2, 100, 10, 64, 16, o, 100)),
               ("tt2_mel_rows", (s, 5, o, c, 2, 3, 0, 4, 1e-5, 0)),
               ("tt2_mel_rows", (o, 5, s, c, 2, 3, 0, 4, 1e-5, 1)),
               ("tt2_mel_rows", (s, 5, o, c, 2, 5, 5, 4, 1e-5, 0))]
    for name, args in refused:
        assert call(name, *args) == _lib.E_INVALID, (name, args)
        assert name.encode() in _lib.load().tt2_last_error(), (name, args)
    torch.cuda.synchronize()
    assert out.untouched()


# ------------------------------------------------------------------ pipeline state (tt2.audio)
def _batch(B, L, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(B, L, generator=g)).to(DEV)


def _nan_fill(P):
    for buf in (P.padded, P.spec, P.mag, P.rows):
        buf.fill_(NAN)


def test_plan_reuse_leaves_no_trace():
    """A loud full-length batch, then a ragged batch of the same shape (one utterance at 513
    samples, what lies beyond each lens[b] loud too) through the same extractor: bit-equal to a fresh
    extractor's result."""
    B, L = 3, 1535
    lens = torch.tensor([L, 513, 1000], dtype=torch.int32, device=DEV)
    used, fresh = MelExtractor(), MelExtractor()
    used(_batch(B, L, 1, scale=50.0))
    x = _batch(B, L, 2)
    for b in range(B):
        x[b, int(lens[b]):] = 77.0
    mel_u, fr_u = used(x, lens)
    mel_f, fr_f = fresh(x, lens)
    assert torch.equal(fr_u, fr_f) and fr_u.tolist() == [6, 3, 4]
    assert torch.equal(mel_u.view(torch.int32), mel_f.view(torch.int32))
    assert (B, L) in used.plans and len(used.plans) == 1


def test_results_do_not_depend_on_plan_buffers():
    """With P.padded, P.spec, P.mag and P.rows NaN-filled before the call (the three tail rows of
    P.spec / P.mag / P.rows are never written, the rows that straddle two utterances are computed
    from both) and NaN beyond every lens[b] of the input, MelExtractor returns the same bits;
    GriffinLim(n_iter = 2) returns the same bits inside every lens[b] and zeros beyond."""
    B, L = 3, 1535
    lens = torch.tensor([L, 513, 1000], dtype=torch.int32, device=DEV)
    mx = MelExtractor()
    x = _batch(B, L, 3)
    mel0, fr0 = mx(x, lens)
    for b in range(B):
        x[b, int(lens[b]):] = NAN
    _nan_fill(mx.plans[(B, L)])
    mel1, fr1 = mx(x, lens)
    assert torch.equal(fr0, fr1)
    assert not torch.isnan(mel1).any()
    assert torch.equal(mel0.view(torch.int32), mel1.view(torch.int32))

    gl = GriffinLim(mx, n_iter=2)
    T = mel0.shape[1]
    y0, l0 = gl(mel0, fr0)
    P = mx.plans[(B, (T - 1) * HOP)]
    _nan_fill(P)
    y1, l1 = gl(mel0, fr0)
    assert torch.equal(l0, l1)
    assert not torch.isnan(y1).any()
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))
    for b in range(B):
        assert y1[b, :int(l1[b])].abs().max().item() > 0
        assert not y1[b, int(l1[b]):].view(torch.int32).any().item(), b


@pytest.mark.parametrize("L", [1280, 1535])
def test_stft_stage(L):
    """MelExtractor.stft at B = 2: L = 1280 gives T = R - 3 and L = 1535 gives T = R - 4, the two
    row-count edges of the plan.  P.padded is bit-equal to the reflect-pad reference; the rows
    [b R, b R + nf_b) of P.spec are held per element to the float64 product of the f32 padded buffer
    and the f32 basis within the GEMM yardstick E = 2 k u |A| |B|^T + 8 u |C| (_gemm_refs.judge_random),
    k = 1024; the padding columns of those rows are +0."""
    B = 2
    lens = np.array([L, 700], dtype=np.int32)
    mx = MelExtractor()
    P = mx.plan(B, L)
    assert P.T == P.R - (3 if L == 1280 else 4)
    _nan_fill(P)
    x = _batch(B, L, L)
    for b in range(B):
        x[b, int(lens[b]):] = NAN
    mx.stft(x, dev(lens), P)
    padded = P.padded.cpu().numpy().reshape(B, P.Lp)
    pp = dict(kernel="reflect_pad", name=f"stft_pad_{L}", exact=True, x=x.cpu().numpy(), lens=lens, batch=B, len=L,
              padded_len=P.Lp, pad=N_FFT // 2)
    hold(pp, padded)
    flat = torch.from_numpy(padded.reshape(-1)).double()
    basis = mx.basis.cpu().double()
    spec = P.spec.cpu()
    worst = 0.0
    for b in range(B):
        nf = 1 + int(lens[b]) // HOP
        r = (b * P.R + torch.arange(nf))[:, None] * HOP + torch.arange(N_FFT)[None, :]
        a = flat[r]
        ref = a @ basis.t()
        e = 2 * N_FFT * G.U * (a.abs() @ basis.abs().t()) + 8 * G.U * ref.abs()
        got = spec[b * P.R:b * P.R + nf]
        fails, w = G.judge_random(got[:, :2 * NB], ref[:, :2 * NB], e[:, :2 * NB])
        assert not fails, (b, fails)
        assert not got[:, 2 * NB:].view(torch.int32).any(), b
        worst = max(worst, w)
    print(f"\nstft stage L = {L}: worst ratio {worst:.3f} of the GEMM yardstick", end="")
    assert LD_SPEC == 2 * NB + 6 and LD_MAG == NB + 3 and N_MELS == 80
