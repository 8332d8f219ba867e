"""Plain references of the five kernels in csrc/audio.hip, written from the contracts in
include/tt2_capi.h (not from the kernels), with the problems the GPU tests run and the judges that
decide them.  Everything runs on the CPU in numpy: float64 is the reference, and the same code
with dtype=float32 (every operation in float32) is the twin that sets the yardstick of the
non-exact checks (_misc_refs.worst_ratio).  tests/test_audio_refs.py pins these against
oracle/tt2_audio_oracle.py and shows, with one deliberately wrong reference per failure mode, that
the judges reject each of them on the very problems tests/test_gpu_audio_kernels.py launches.

A problem is a dict: the kernel's name ("kernel"), a label ("name"), the inputs as the kernel gets
them (leading dimensions included; whatever the kernel must not read is NaN), the scalar
arguments, and "exact" (bit equality) or not (worst_ratio <= 1, or the ulp bar in "ulps").
`reference(p, dtype, mutant)` evaluates it; `judge(p, got)` returns (ok, text)."""
import numpy as np
import torch

import _misc_refs as R

F32, F64 = np.float32, np.float64
NAN = float("nan")
GRID_CAP = 16384 * 256           # elements one trip of every kernel's grid-stride loop covers
WSS_EPS = 1e-8                   # overlap-add: a divisor at or below this gives 0


def eff_len(lens, b, cap):
    """lens[b] limited to cap (the header: lens[b] > len counts as len); cap where lens is None."""
    return cap if lens is None else min(int(lens[b]), cap)


# ------------------------------------------------------------------ reflect padding
def ref_reflect_pad(p, dtype=F64, mutant=None):
    """padded[b][j] = x[b][reflect(j - pad)] for j < len_b + 2 pad, 0 beyond: np.pad "reflect" where
    len_b > pad; for 0 < len_b <= pad one reflection each side, then clamped into [0, len_b) (the
    header's rule; np.pad reflects again and again instead); all zero for len_b <= 0."""
    x, lens, L, Lp, pad = p["x"], p["lens"], p["len"], p["padded_len"], p["pad"]
    B = p["batch"]
    out = np.zeros((B, Lp), dtype=x.dtype)          # a move: the input's own type
    for b in range(B):
        n = eff_len(lens if mutant != "next_lens" else np.roll(np.asarray(lens), -1), b, L) \
            if lens is not None else L
        if n <= 0:
            continue
        row = x[b, :n]
        if n > pad and mutant is None:
            out[b, :n + 2 * pad] = np.pad(row, pad, mode="reflect")
            continue
        if mutant == "symmetric" and n > pad:
            out[b, :n + 2 * pad] = np.pad(row, pad, mode="symmetric")
            continue
        s = np.arange(Lp if mutant == "tail_kept" else n + 2 * pad) - pad
        s = np.where(s < 0, -s, s)
        s = np.where(s >= n, (2 * n if mutant == "right_about_len" else 2 * (n - 1)) - s, s)
        out[b, :len(s)] = row[np.clip(s, 0, n - 1)]
    return out


def _pad_problem(name, pad, L, Lp, lens, ldx, batch=None):
    B = len(lens) if lens is not None else batch
    x = np.full((B, ldx), NAN, dtype=F32)
    for b in range(B):
        n = max(0, eff_len(lens, b, L))
        x[b, :n] = 1 + b * 4099 + np.arange(n)       # every sample its own integer (< 2^24)
    return dict(kernel="reflect_pad", name=name, exact=True, x=x, lens=None if lens is None else
                np.asarray(lens, dtype=np.int32), batch=B, len=L, padded_len=Lp, pad=pad, ldx=ldx)


def ragged_lens(L, pad):
    return [L, L - 1, pad + 1, pad, 1, 0, -3, L + 7]


def reflect_pad_problems():
    ps = []
    for pad, L, Lp in [(4, 9, 24), (512, 1300, 2560), (512, 513, 1792)]:
        g = f"pad{pad}_len{L}_lp{Lp}"
        ps.append(_pad_problem(g + "_ragged", pad, L, Lp, ragged_lens(L, pad), L))
        ps.append(_pad_problem(g + "_ragged_ldx", pad, L, Lp, ragged_lens(L, pad), L + 5))
        ps.append(_pad_problem(g + "_nolens", pad, L, Lp, None, L + 5, batch=3))
    return ps


def reflect_pad_grid_problem():
    """B * padded_len just above one trip of the loop; two utterances so that b and j both change
    in the second trip."""
    L = GRID_CAP // 2 + 37
    return _pad_problem("grid_stride", 4, L, L + 8 + 3, [L, L - 5], L + 1)


# ------------------------------------------------------------------ magnitude
def ref_spec_magnitude(p, dtype=F64, mutant=None):
    """mag[r][k] = sqrt(re^2 + im^2), k < n_bins; +0 in [n_bins, ld_mag)."""
    nb = p["n_bins"]
    spec = p["spec"].astype(dtype)
    re, im = spec[:, :nb], spec[:, nb:2 * nb]
    out = np.zeros((p["m"], p["ld_mag"]), dtype=dtype)
    out[:, :nb] = np.sqrt(re * re) if mutant == "no_imag" else np.sqrt(re * re + im * im)
    return out


PYTHAGOREAN = [(3, 4), (5, 12), (8, 15), (7, 24), (20, 21), (9, 40), (12, 35), (28, 45), (0, 7), (7, 0), (0, 0)]


def _spec_buffer(m, ld_spec):
    """[m, ld_spec] of NaN: the columns at and beyond 2 n_bins stay that way."""
    return np.full((m, ld_spec), NAN, dtype=F32)


def magnitude_problems():
    ps = []
    for nb in (1, 5, 513):
        for ld_mag in (nb, nb + 3):
            for ld_spec in (2 * nb, 2 * nb + 6):
                rng = np.random.default_rng(nb * 100 + ld_mag + ld_spec)
                m = 7
                base = dict(kernel="spec_magnitude", m=m, n_bins=nb, ld_mag=ld_mag, ld_spec=ld_spec)
                tag = f"nb{nb}_ldm{ld_mag}_lds{ld_spec}"
                # selector: Pythagorean pairs and (x, 0) / (0, x), signs and powers of two varied
                pairs = np.array(PYTHAGOREAN)[rng.integers(0, len(PYTHAGOREAN), (m, nb))]
                swap = rng.integers(0, 2, (m, nb)).astype(bool)
                scale = np.ldexp(1.0, rng.integers(-6, 7, (m, nb)))
                a = np.where(swap, pairs[..., 1], pairs[..., 0]) * scale * rng.choice([-1, 1], (m, nb))
                b = np.where(swap, pairs[..., 0], pairs[..., 1]) * scale * rng.choice([-1, 1], (m, nb))
                spec = _spec_buffer(m, ld_spec)
                spec[:, :nb], spec[:, nb:2 * nb] = a, b
                ps.append(dict(base, name="selector_" + tag, exact=True, spec=spec))
                # random: magnitudes from 2^-40 to 2^40, the two parts up to 2^6 apart
                spec = _spec_buffer(m, ld_spec)
                e = rng.uniform(-40, 40, (m, nb))
                spec[:, :nb] = rng.standard_normal((m, nb)) * np.exp2(e)
                spec[:, nb:2 * nb] = rng.standard_normal((m, nb)) * np.exp2(e + rng.uniform(-6, 6, (m, nb)))
                ps.append(dict(base, name="random_" + tag, exact=False, ulps=2, spec=spec))
    return ps


def magnitude_grid_problem():
    """m * ld_mag just above one trip; integer-valued (Pythagorean) inputs: bit-exact."""
    nb, ld_mag, ld_spec = 5, 8, 10
    m = GRID_CAP // ld_mag + 3
    r = np.arange(m)[:, None] + np.arange(nb)[None, :]
    pairs = np.array(PYTHAGOREAN)[r % len(PYTHAGOREAN)]
    spec = np.zeros((m, ld_spec), dtype=F32)
    spec[:, :nb], spec[:, nb:2 * nb] = pairs[..., 0], -pairs[..., 1]
    return dict(kernel="spec_magnitude", name="grid_stride", exact=True, m=m, n_bins=nb, ld_mag=ld_mag,
                ld_spec=ld_spec, spec=spec)


# ------------------------------------------------------------------ rephase
def ref_spec_rephase(p, dtype=F64, mutant=None):
    """out[r][k], out[r][n_bins + k] = mag[r][k] * e / |e|, e = est[r][k] + i est[r][n_bins + k];
    phase 0 (re = mag, im = +0 * mag) where est is None or e == 0; +0 in [2 n_bins, ld_out)."""
    nb, m = p["n_bins"], p["m"]
    mag = p["mag"][:, :nb].astype(dtype)
    out = np.zeros((m, p["ld_out"]), dtype=dtype)
    c, s = np.ones_like(mag), np.zeros_like(mag)
    if p["est"] is not None:
        est = p["est"].astype(dtype)
        re, im = est[:, :nb], est[:, nb:2 * nb]
        if mutant == "swap":
            re, im = im, re
        if mutant == "conj":
            im = -im
        a = np.sqrt(re * re + im * im)
        ok = a > 0
        safe = np.where(ok, a, 1)
        reset = (0, 0) if mutant == "no_reset" else (1, 0)
        c, s = np.where(ok, re / safe, reset[0]).astype(dtype), np.where(ok, im / safe, reset[1]).astype(dtype)
    out[:, :nb], out[:, nb:2 * nb] = mag * c, mag * s
    return out


def rephase_problems():
    ps = []
    for nb in (7, 513):                      # 2 n_bins + 6 <= 3 n_bins needs n_bins >= 6
        for ld_out in (2 * nb, 2 * nb + 6, 3 * nb):
            for ld_mag, ld_est in ((nb, 2 * nb), (nb + 3, 2 * nb + 6)):
                rng = np.random.default_rng(nb + ld_out + ld_mag)
                m = 6
                base = dict(kernel="spec_rephase", m=m, n_bins=nb, ld_mag=ld_mag, ld_est=ld_est, ld_out=ld_out)
                tag = f"nb{nb}_ldo{ld_out}_ldm{ld_mag}"
                mag = np.full((m, ld_mag), NAN, dtype=F32)
                mag[:, :nb] = np.abs(rng.standard_normal((m, nb))) * np.exp2(rng.uniform(-20, 20, (m, nb)))
                mag[0, 0] = 0.0
                ps.append(dict(base, name="null_est_" + tag, exact=True, mag=mag, est=None))
                # est on an axis, (+-x, 0) or (0, +-x), or exactly zero: +-mag, bit for bit
                est = np.full((m, ld_est), NAN, dtype=F32)
                x = (np.abs(rng.standard_normal((m, nb))) * np.exp2(rng.uniform(-30, 30, (m, nb)))).astype(F32)
                kind = rng.integers(0, 5, (m, nb))          # 0: +re, 1: -re, 2: +im, 3: -im, 4: e == 0
                kind[1, 0] = 4
                est[:, :nb] = np.where(kind == 0, x, np.where(kind == 1, -x, 0))
                est[:, nb:2 * nb] = np.where(kind == 2, x, np.where(kind == 3, -x, 0))
                ps.append(dict(base, name="axis_est_" + tag, exact=True, mag=mag, est=est))
                est = np.full((m, ld_est), NAN, dtype=F32)
                e = rng.uniform(-40, 40, (m, nb))
                est[:, :nb] = rng.standard_normal((m, nb)) * np.exp2(e)
                est[:, nb:2 * nb] = rng.standard_normal((m, nb)) * np.exp2(e + rng.uniform(-6, 6, (m, nb)))
                ps.append(dict(base, name="random_" + tag, exact=False, ulps=3, mag=mag, est=est))
    return ps


def rephase_grid_problem():
    """m * n_bins just above one trip; est on the axes: bit-exact."""
    nb, ld_mag, ld_est, ld_out = 4, 4, 8, 10
    m = GRID_CAP // nb + 3
    i = np.arange(m)[:, None] * nb + np.arange(nb)[None, :]
    mag = (1 + i % 1021).astype(F32)
    est = np.zeros((m, ld_est), dtype=F32)
    kind = i % 5
    est[:, :nb] = np.where(kind == 0, 2.0, np.where(kind == 1, -3.0, 0))
    est[:, nb:2 * nb] = np.where(kind == 2, 5.0, np.where(kind == 3, -0.5, 0))
    return dict(kernel="spec_rephase", name="grid_stride", exact=True, m=m, n_bins=nb, ld_mag=ld_mag,
                ld_est=ld_est, ld_out=ld_out, mag=mag, est=est)


# ------------------------------------------------------------------ overlap-add
def hann(n_fft, dtype=F64, form="sin2"):
    """Periodic Hann window of n_fft points.  float64: the definition.  float32 forms, every
    operation in float32: "sin2" = sin^2(pi n / n_fft), with the argument folded to
    pi min(n, n_fft - n) / n_fft (the same function: the window is symmetric about n_fft / 2),
    so that it stays within [0, pi / 2] where the sine is as accurate in relative terms as its
    argument; "cos" = 0.5 - 0.5 cos(2 pi n / n_fft), which cancels near both ends of the window;
    "symmetric" = the non-periodic window (denominator n_fft - 1), a mutant."""
    n = np.arange(n_fft)
    if form == "symmetric":
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / (n_fft - 1))).astype(dtype)
    if dtype == F64:
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)
    if form == "cos":
        w0 = F32(6.283185307179586) / F32(n_fft)
        return F32(0.5) - F32(0.5) * np.cos(w0 * n.astype(F32), dtype=F32)
    w0 = F32(3.141592653589793) / F32(n_fft)
    s = np.sin(w0 * np.minimum(n, n_fft - n).astype(F32), dtype=F32)
    return s * s


def ref_overlap_add(p, dtype=F64, mutant=None, form="sin2", want_wss=False):
    """y[b][t] = sum_f frames[b * R + f][n] / sum_f hann^2[n], n = t + n_fft / 2 - f hop, over the
    frames f < nf_b = 1 + len_b // hop with 0 <= n < n_fft, for t < len_b; 0 where the divisor is
    at most 1e-8 and for t >= len_b.  Sums run in increasing f, in `dtype`."""
    fr, lens, L, R = p["frames"], p["lens"], p["len"], p["rows_per_utt"]
    n_fft, hop, B = p["n_fft"], p["hop"], p["batch"]
    pad = 0 if mutant == "centre_kept" else n_fft // 2
    w = hann(n_fft, dtype, "symmetric" if mutant == "symmetric_hann" else form)
    w2 = w if mutant == "unsquared" else w * w
    K = -(-n_fft // hop)
    y = np.zeros((B, L), dtype=dtype)
    wss_all = np.zeros((B, L), dtype=dtype)
    for b in range(B):
        n_b = eff_len(lens, b, L)
        if n_b <= 0:
            continue
        nf = n_b // hop if mutant == "nf_no_plus_1" else 1 + n_b // hop
        j = np.arange(n_b) + pad
        acc, wss = np.zeros(n_b, dtype=dtype), np.zeros(n_b, dtype=dtype)
        f_first = np.maximum(0, -(-(j - n_fft + 1) // hop))          # first f with f hop + n_fft > j
        f_last = np.minimum(nf - 1, j // hop)
        if mutant == "first_dropped":
            f_first = f_first + 1
        if mutant == "last_dropped":
            f_last = f_last - 1
        for k in range(K - 1, -1, -1):                               # increasing f
            f = j // hop - k
            n = j - f * hop
            ok = (f >= f_first) & (f <= f_last) & (n < n_fft)
            fc, nc = np.clip(f, 0, R - 1), np.clip(n, 0, n_fft - 1)
            acc = acc + np.where(ok, fr[b * R + fc, nc].astype(dtype), 0).astype(dtype)
            wss = wss + np.where(ok, w2[nc], 0).astype(dtype)
        y[b, :n_b] = np.where(wss > dtype(WSS_EPS), acc / np.where(wss > 0, wss, 1), 0)
        wss_all[b, :n_b] = wss
    return (y, wss_all) if want_wss else y


OLA_GEOMETRIES = [(1024, 256), (64, 16), (64, 32), (64, 64), (48, 20), (9, 4)]


def ola_shape(n_fft, hop):
    """(len, rows_per_utt) of the problems at one geometry: a few frames, rows beyond the contract's
    minimum (rows_per_utt * hop >= len + n_fft)."""
    L = 5 * hop + hop // 2 + 3
    return L, -(-(L + n_fft) // hop) + 1


def ola_lens(L, hop):
    return [3 * hop, 2 * hop + hop - 1, 1, 0, L, L + 5]


def _ola_base(n_fft, hop, lens, ld_frames):
    L, Rr = ola_shape(n_fft, hop)
    B = len(lens)
    return dict(kernel="overlap_add", batch=B, len=L, rows_per_utt=Rr, n_fft=n_fft, hop=hop, ld_frames=ld_frames,
                lens=np.asarray(lens, dtype=np.int32))


def ola_random_problem(n_fft, hop):
    """Seeded frames; rows at f >= nf_b (straddle rows among them) and columns beyond n_fft NaN."""
    L, Rr = ola_shape(n_fft, hop)
    lens = ola_lens(L, hop)
    p = _ola_base(n_fft, hop, lens, n_fft + 3)
    rng = np.random.default_rng(n_fft * 131 + hop)
    fr = np.full((p["batch"] * Rr, n_fft + 3), NAN, dtype=F32)
    for b in range(p["batch"]):
        n_b = eff_len(lens, b, L)
        if n_b > 0:
            nf = 1 + n_b // hop
            fr[b * Rr:b * Rr + nf, :n_fft] = rng.standard_normal((nf, n_fft))
    return dict(p, name=f"random_{n_fft}_{hop}", exact=False, frames=fr)


def ola_onehot_cells(n_fft, hop):
    """(b, f, n) of every one-hot cell walked at one geometry: the first and last utterance of
    ola_lens-shaped batches, f in {0, 1, nf - 1, nf} (nf: must not appear), n at the window's and the
    hop's edges."""
    L, _ = ola_shape(n_fft, hop)
    lens = [3 * hop + 1, 2 * hop + hop - 1, L]
    cells = []
    for b in (0, len(lens) - 1):
        nf = 1 + min(lens[b], L) // hop
        for f in sorted({0, 1, nf - 1, nf}):
            for n in sorted({0, 1, hop - 1, min(hop, n_fft - 1), n_fft - 1}):
                cells.append((b, f, n))
    return lens, cells


def ola_onehot_problem(n_fft, hop, lens, cell):
    p = _ola_base(n_fft, hop, lens, n_fft)
    fr = np.zeros((p["batch"] * p["rows_per_utt"], n_fft), dtype=F32)
    b, f, n = cell
    fr[b * p["rows_per_utt"] + f, n] = 1.0
    return dict(p, name=f"onehot_{n_fft}_{hop}_b{b}_f{f}_n{n}", exact=False, onehot=cell, frames=fr)


def ola_onehot_expected(p):
    """(b, t) of the one sample that may be nonzero, or None when the cell must not appear at all
    (a frame at or beyond nf_b, or a sample outside [0, len_b))."""
    b, f, n = p["onehot"]
    n_b = eff_len(p["lens"], b, p["len"])
    t = f * p["hop"] + n - p["n_fft"] // 2
    if n_b <= 0 or f >= 1 + n_b // p["hop"] or not 0 <= t < n_b:
        return None
    return b, t


def ola_grid_problem():
    """batch * len just above one trip; integer-valued frames (|v| <= 4)."""
    n_fft, hop = 8, 4
    L = GRID_CAP // 2 + 21
    Rr = -(-(L + n_fft) // hop)
    lens = [L, L - 6]
    i = np.arange(2 * Rr)[:, None] * 3 + np.arange(n_fft)[None, :]
    fr = ((i % 9) - 4).astype(F32)
    return dict(kernel="overlap_add", name="grid_stride", exact=False, batch=2, len=L, rows_per_utt=Rr, n_fft=n_fft,
                hop=hop, ld_frames=n_fft, lens=np.asarray(lens, dtype=np.int32), frames=fr)


def ola_borderline(p):
    """Number of compared samples whose float64 divisor lies within a factor 2 of the 1e-8 threshold
    (where float32 and float64 could take different sides of it)."""
    _, wss = ref_overlap_add(p, F64, want_wss=True)
    valid = np.zeros_like(wss, dtype=bool)
    for b in range(p["batch"]):
        valid[b, :max(0, eff_len(p["lens"], b, p["len"]))] = True
    return int(((wss > WSS_EPS / 2) & (wss < WSS_EPS * 2) & valid).sum())


# ------------------------------------------------------------------ mel rows
def _nf(frames, b, T):
    return T if frames is None else max(0, min(int(frames[b]), T))


def ref_mel_gather(p, dtype=F64, mutant=None):
    """mel[b][t][c] = log(max(rows[b * R + t][c], clamp)) for t < nf_b = min(frames[b], T), else
    log(clamp); frames[b] <= 0: all silence."""
    B, T, C, Rr = p["batch"], p["t"], p["n_mels"], p["rows_per_utt"]
    clamp = dtype(F32(p["clamp"]))
    out = np.full((B, T, C), 0.0 if mutant == "silence_zero" else np.log(clamp), dtype=dtype)
    for b in range(B):
        nf = _nf(p["frames"], b, T)
        v = p["rows"][b * Rr:b * Rr + nf, :C].astype(dtype)
        if mutant == "log_before_clamp":
            with np.errstate(all="ignore"):
                out[b, :nf] = np.fmax(np.log(v), clamp)
        else:
            out[b, :nf] = np.log(np.maximum(v, clamp))
    return out


def ref_mel_scatter(p, dtype=F64, mutant=None):
    """rows[b * R + t][c] = exp(mel[b][t][c]) for t < nf_b, +0 for nf_b <= t < R; columns at and
    beyond n_mels are not the kernel's (NaN here: never compared)."""
    B, T, C, Rr = p["batch"], p["t"], p["n_mels"], p["rows_per_utt"]
    out = np.zeros((B * Rr, C), dtype=dtype)
    for b in range(B):
        nf = T if mutant == "scatter_no_zero" else _nf(p["frames"], b, T)
        with np.errstate(all="ignore"):
            out[b * Rr:b * Rr + nf] = np.exp(p["mel"][b, :nf].astype(dtype))
    return out


def mel_frames(T):
    return [None, [T] * 6, [T, T + 3, 1, 0, -2, max(1, T - 1)]]


def mel_rows_problems():
    ps = []
    Rr, C = 9, 5
    for T in (1, Rr, Rr - 3):
        for ld_rows in (C, C + 4):
            for fi, frames in enumerate(mel_frames(T)):
                B = 6
                rng = np.random.default_rng(T * 100 + ld_rows * 10 + fi)
                fr = None if frames is None else np.asarray(frames, dtype=np.int32)
                base = dict(batch=B, t=T, n_mels=C, rows_per_utt=Rr, ld_rows=ld_rows, clamp=1e-5, frames=fr)
                tag = f"t{T}_ld{ld_rows}_frames{fi}"
                rows = np.full((B * Rr, ld_rows), NAN, dtype=F32)
                mel = np.full((B, T, C), NAN, dtype=F32)
                for b in range(B):
                    nf = _nf(fr, b, T)
                    v = np.exp(rng.uniform(np.log(1e-12), np.log(1e6), (nf, C)))
                    special = np.array([F32(1e-5), 0.0, -3.5, 1.0, np.nextafter(F32(1e-5), F32(1)), -0.0])
                    pick = rng.integers(0, 3 * len(special), (nf, C))
                    v = np.where(pick < len(special), special[pick % len(special)], v)
                    rows[b * Rr:b * Rr + nf, :C] = v
                    mel[b, :nf] = rng.uniform(-12, 6, (nf, C))
                ps.append(dict(base, kernel="mel_gather", name="gather_" + tag, exact=False, rows=rows))
                ps.append(dict(base, kernel="mel_scatter", name="scatter_" + tag, exact=False, mel=mel))
    return ps


def mel_rows_grid_problems():
    """batch * rows_per_utt * n_mels just above one trip.  Gather of 1.0 / clamp / below: log is 0 or
    log(clamp); scatter of 0 / -inf: exp is 1 or 0 (bit-exact on any correct exp)."""
    C, Rr, T = 8, 64, 61
    B = GRID_CAP // (C * Rr) + 1
    frames = np.where(np.arange(B) % 3 == 0, T - 2, T).astype(np.int32)
    i = np.arange(B * Rr)[:, None] + np.arange(C)[None, :]
    rows = np.where(i % 3 == 0, 1.0, np.where(i % 3 == 1, 1e-7, -2.0)).astype(F32)
    base = dict(batch=B, t=T, n_mels=C, rows_per_utt=Rr, ld_rows=C, clamp=1e-5, frames=frames, exact=False)
    j = np.arange(B * T * C).reshape(B, T, C)
    mel = np.where(j % 2 == 0, 0.0, -np.inf).astype(F32)
    return [dict(base, kernel="mel_gather", name="grid_stride_gather", rows=rows),
            dict(base, kernel="mel_scatter", name="grid_stride_scatter", mel=mel)]


# ------------------------------------------------------------------ dispatch and judges
REFS = {"reflect_pad": ref_reflect_pad, "spec_magnitude": ref_spec_magnitude, "spec_rephase": ref_spec_rephase,
        "overlap_add": ref_overlap_add, "mel_gather": ref_mel_gather, "mel_scatter": ref_mel_scatter}


def reference(p, dtype=F64, mutant=None, **kw):
    return REFS[p["kernel"]](p, dtype, mutant, **kw)


def as_output(a):
    """What a kernel that computed `a` would store: float32."""
    return np.asarray(a).astype(F32)


def bits_equal(got, want):
    g, w = (torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).view(torch.int32) for a in (got, want))
    return torch.equal(g, w)


def ulp_ratio(got, ref64, ulps):
    """max |got - ref64| / (ulps * f32 ulp at |ref64|)."""
    g, r = (torch.from_numpy(np.asarray(a, dtype=F64)).reshape(-1) for a in (got, ref64))
    if r.numel() == 0:
        return 0.0
    err = (g - r).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return (err / (ulps * R.ulp(r, torch.float32))).max().item()


def judge(p, got):
    """(ok, text) for a kernel's output `got` (float32, the logical extent reference() returns).
    exact problems: bit equality with the float64 reference cast to float32.  "ulps" problems: every
    element within that many f32 ulp of the float64 reference (and, for the rephase, the modulus
    within the same bar of the magnitude).  Others: worst_ratio <= 1 through the float32 twin."""
    ref64 = reference(p, F64)
    got = np.ascontiguousarray(got, dtype=F32)
    if got.shape != ref64.shape:
        return False, f"shape {got.shape}, expected {ref64.shape}"
    if p["exact"]:
        ok = bits_equal(got, as_output(ref64))
        return ok, "bit-equal" if ok else f"{int((got.view(np.int32) != as_output(ref64).view(np.int32)).sum())} " \
                                          "elements differ in bits"
    if "ulps" in p:
        ratio = ulp_ratio(got, ref64, p["ulps"])
        text = f"ratio {ratio:.3f} of {p['ulps']} ulp"
        if p["kernel"] == "spec_rephase":
            nb = p["n_bins"]
            g = got.astype(F64)
            mag = p["mag"][:, :nb].astype(F64)
            m2 = g[:, :nb] ** 2 + g[:, nb:2 * nb] ** 2
            allowed = 2 * mag * p["ulps"] * R.ulp(torch.from_numpy(mag), torch.float32).numpy()
            with np.errstate(all="ignore"):
                r2 = np.where(allowed > 0, np.abs(m2 - mag * mag) / np.where(allowed > 0, allowed, 1), 0.0)
            r2 = float(np.nan_to_num(r2, nan=np.inf).max())
            text += f", modulus ratio {r2:.3f}"
            ratio = max(ratio, r2)
        return ratio <= 1.0, text
    ref32 = reference(p, F32)
    with np.errstate(all="ignore"):
        ratio = R.worst_ratio(torch.from_numpy(got.astype(F64)), torch.from_numpy(ref64),
                              torch.from_numpy(ref32.astype(F64)))
    if p["kernel"] in ("overlap_add", "mel_scatter"):
        # what the contract makes exactly +0 (beyond len_b, a divisor at most 1e-8, rows at and beyond
        # frames[b], and sums of zeros) is held to those bits, not to the yardstick
        zero = (ref64 == 0) & (ref32 == 0)
        if (got[zero].view(np.int32) != 0).any():
            return False, f"{int((got[zero].view(np.int32) != 0).sum())} elements that must be +0 are not"
    return ratio <= 1.0, R.describe(torch.from_numpy(got.astype(F64)), torch.from_numpy(ref64),
                                    torch.from_numpy(ref32.astype(F64)))
