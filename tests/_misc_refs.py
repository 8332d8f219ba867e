"""Plain references of the HBM-bound kernels in csrc/reduce.hip, embed.hip, loss.hip, optim.hip
and repack.hip, written from the contracts in
include/tt2_capi.h (not from the kernels).  Everything runs on the CPU in float64 unless a
`dtype` is given: the same code in float32 is the yardstick of the non-exact checks
(`worst_ratio`).  tests/test_misc_refs.py validates these against independent
implementations (torch autograd, torch.optim, the oracle's tts_loss)."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


# ------------------------------------------------------------------ embedding
def ref_embedding_fwd(ids, table, vocab):
    """out[m] = table[ids[m]], a zero row for ids outside [0, vocab); table's own dtype."""
    ids = ids.long()
    ok = (ids >= 0) & (ids < vocab)
    out = table[ids.clamp(0, vocab - 1)].clone()
    out[~ok] = 0
    return out


def ref_embedding_bwd(ids, dout, vocab, pad_idx):
    """dtable[v] = sum of the dout rows with ids == v in float64; row pad_idx is zero and ids
    outside [0, vocab) contribute nothing."""
    ids = ids.long()
    ok = (ids >= 0) & (ids < vocab) & (ids != pad_idx)
    dt = torch.zeros(vocab, dout.shape[-1], dtype=F64)
    dt.index_add_(0, ids[ok], dout.to(F64)[ok])
    return dt


def ref_embedding_bwd_f32_ordered(ids, dout, vocab, pad_idx):
    """The same sum added in float32 in increasing row order: the order the header promises,
    so this is the bit-exact expectation for any input."""
    ids = ids.long().numpy()
    d = dout.float().numpy()
    dt = np.zeros((vocab, d.shape[-1]), dtype=np.float32)
    for m in range(ids.shape[0]):
        v = ids[m]
        if 0 <= v < vocab and v != pad_idx:
            dt[v] += d[m]
    return torch.from_numpy(dt)


# ------------------------------------------------------ positional encoding
def ref_posenc_bwd(dout, pe, T, keep, scale, dtype=F64):
    """dx = drop'(dout) = keep ? dout * scale : 0 and dalpha = sum(dx * pe[row % T]).
    dout [M, C]; pe [>= T, C]; keep: bool [M, C] or None (no dropout, scale 1)."""
    d = dout.to(dtype)
    dx = d if keep is None else torch.where(keep, d * scale, torch.zeros((), dtype=dtype))
    rows = torch.arange(d.shape[0]) % T
    dalpha = (dx * pe.to(dtype)[rows]).sum()
    return dx, dalpha


# ---------------------------------------------------- teacher forcing, sums
def ref_shift_right(mel):
    """mel f32 [B, T, C] -> [B * T, C]: row (b, t) = mel[b, t - 1], zero at t == 0."""
    B, T, C = mel.shape
    out = torch.zeros_like(mel)
    out[:, 1:] = mel[:, :-1]
    return out.reshape(B * T, C)


def ref_colsum(x, beta, dst0):
    """dst[n] = beta * dst0[n] + sum_m x[m, n] in float64 (x: the logical [m, n] matrix).
    beta == 0 ignores dst0 (it may hold anything)."""
    s = x.to(F64).sum(0)
    return s if beta == 0 else beta * dst0.to(F64) + s


ref_reduce_rows = ref_colsum   # dst[c] = beta * dst[c] + sum_r src[r, c]: the same contract on f32


def ref_sumsq(g):
    return (g.to(F64) ** 2).sum()


# --------------------------------------------------------------------- loss
def ref_tts_loss(heads, after, target, mel_len, n_mels, pos_weight=5.0, grad_scale=1.0, separate=False,
                 dtype=F64):
    """heads [B*T, heads_ld] (cols < n_mels: mel_before, col n_mels: stop logit, the rest unused),
    after [B*T, n_mels], target [B, T, n_mels], mel_len [B].

    Frame (b, t) is valid iff t < mel_len[b]; N = sum_b clamp(mel_len[b], 0, T) valid frames.
    The stop label is 1 at t == mel_len[b] - 1 (no frame of a sequence cut off at T carries it).
    loss = (total, mse_before, mse_after, bce_stop), the means over the valid frames (N == 0: all
    zero).  Gradients are those of `total` times grad_scale; g_heads [B*T, heads_ld] has the stop
    column at n_mels, zeros above it, and in its mel columns d/d(before) (+ d/d(after) unless
    `separate`); g_after [B*T, n_mels].  Padded frames and N == 0 give zero gradients."""
    B, T, NM = target.shape
    assert NM == n_mels
    ln = mel_len.long()
    t = torch.arange(T)[None, :]
    valid = (t < ln[:, None]).reshape(-1)                      # [B*T]
    y = (t == (ln[:, None] - 1)).reshape(-1).to(dtype)
    N = int(ln.clamp(0, T).sum())
    h = heads.to(dtype)
    tg = target.to(dtype).reshape(B * T, NM)
    db = h[:, :NM] - tg
    da = after.to(dtype) - tg
    x = h[:, NM]
    n = max(N, 1)
    zero = torch.zeros((), dtype=dtype)
    l_b = torch.where(valid[:, None], db * db, zero).sum() / (n * NM)
    l_a = torch.where(valid[:, None], da * da, zero).sum() / (n * NM)
    bce = -(pos_weight * y * F.logsigmoid(x) + (1 - y) * F.logsigmoid(-x))
    l_s = torch.where(valid, bce, zero).sum() / n
    loss = torch.stack([l_b + l_a + l_s, l_b, l_a, l_s])
    inv_n = grad_scale / N if N > 0 else 0.0
    g_b = torch.where(valid[:, None], 2 * db * (inv_n / NM), zero)
    g_a = torch.where(valid[:, None], 2 * da * (inv_n / NM), zero)
    s = torch.sigmoid(x)
    g_s = torch.where(valid, (pos_weight * y * (s - 1) + (1 - y) * s) * inv_n, zero)
    g_heads = torch.zeros(B * T, heads.shape[1], dtype=dtype)
    g_heads[:, :NM] = g_b if separate else g_b + g_a
    g_heads[:, NM] = g_s
    return loss, g_heads, g_a


# --------------------------------------------------------------------- Adam
def ref_adam(p, g, m, v, step, lr, beta1=0.9, beta2=0.98, eps=1e-9, weight_decay=0.0, clip_norm=1.0,
             warmup=4000.0, noam=True, d_model=512, dtype=F64):
    """One step (`step` = its 1-based number) of decoupled-weight-decay Adam with global-norm
    clipping (g *= clip / (norm + 1e-6) when norm > clip) and the Noam schedule
    lr * d_model^-0.5 * min(step^-0.5, step * warmup^-1.5).  Returns the new (p, m, v)."""
    p, g, m, v = (a.to(dtype) for a in (p, g, m, v))
    sc = lambda a: torch.tensor(a, dtype=dtype)   # noqa: E731  (scalars in the working precision too)
    if clip_norm > 0:
        nrm = (g * g).sum().sqrt()
        if nrm > clip_norm:
            g = g * (sc(clip_norm) / (nrm + sc(1e-6)))
    st = sc(float(step))
    rate = sc(lr)
    if noam:
        rate = rate * sc(float(d_model)) ** -0.5 * torch.minimum(st ** -0.5, st * sc(warmup) ** -1.5)
    if weight_decay != 0:
        p = p - rate * sc(weight_decay) * p
    m = sc(beta1) * m + (1 - sc(beta1)) * g
    v = sc(beta2) * v + (1 - sc(beta2)) * g * g
    bc1 = 1 - sc(beta1) ** st
    bc2 = 1 - sc(beta2) ** st
    p = p - (rate / bc1) * m / (v.sqrt() / bc2.sqrt() + sc(eps))
    return p, m, v


# ------------------------------------------------- the non-exact yardstick
def ulp(ref, out_dtype):
    """Spacing of out_dtype at |ref|'s magnitude (at least the smallest normal's)."""
    bits = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}[out_dtype]
    _, e = torch.frexp(ref.to(F64).abs().clamp_min(2.0 ** -126))   # |ref| = f * 2^e, f in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref, dtype=F64), e - 1 - bits)


def worst_ratio(got, ref64, ref32, out_dtype=torch.float32):
    """max over elements of |got - ref64| / max(4 * E32, 2 ulp(out_dtype at |ref64|)), where
    E32 = max |ref32 - ref64| is the worst error of the same reference evaluated in float32 on
    the CPU, over the tensor compared: <= 1 passes.

    E32 is taken over the tensor, not element by element: the float32 error of one element is a
    single draw of a rounding error whose scale the element's neighbours share, and a kernel that
    rounds in another (fixed) order draws again, so element i's own draw (often 0) says little about
    the error a correct kernel may show there.  For a scalar the two readings coincide."""
    got, ref64, ref32 = (torch.as_tensor(a).to(F64).cpu().reshape(-1) for a in (got, ref64, ref32))
    if ref64.numel() == 0:
        return 0.0
    allowed = torch.clamp_min(2 * ulp(ref64, out_dtype), 4 * (ref32 - ref64).abs().max().item())
    err = (got - ref64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return (err / allowed).max().item()


def describe(got, ref64, ref32, out_dtype=torch.float32):
    """'ratio R (err E ulp, f32 reference F ulp)': worst_ratio and, in ulps of out_dtype at the
    element where the ratio is worst, the kernel's error and the float32 reference's worst error."""
    g, r, r32 = (torch.as_tensor(a).to(F64).cpu().reshape(-1) for a in (got, ref64, ref32))
    if r.numel() == 0:
        return "ratio 0 (empty)"
    u = ulp(r, out_dtype)
    e32 = (r32 - r).abs().max()
    ratio = (g - r).abs() / torch.clamp_min(2 * u, 4 * e32.item())
    i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
    return (f"ratio {worst_ratio(got, ref64, ref32, out_dtype):.3f} (err {((g - r).abs() / u)[i].item():.2f} ulp, "
            f"f32 reference {(e32 / u[i]).item():.2f} ulp)")


# exact-arithmetic inputs: integer-valued terms (or a common power-of-two multiple of integers)
# whose absolute values sum to less than 2^24 make every partial sum exact in f32, whatever the
# order; the tests assert this bound on the inputs they choose
EXACT_LIMIT = 2.0 ** 24
