"""CPU: the references of tests/_upsample_refs.py against torch float64 autograd of ESPnet's composed
form and of Non-Attentive Tacotron's, the premises of the exact problems the GPU tests compare bit for
bit, and that the bar of the GPU tests (judge) rejects each of the twelve mutants, over every row and
confined to one 32-row tile."""
import numpy as np
import pytest
import torch

import _upsample_refs as R

F64 = torch.float64


def composed(h, c, prec, bias, offset, n_out, tx_b):
    """The torch form, ESPnet's GaussianUpsampling generalised by a bias: arange, a broadcast square,
    masked_fill, softmax, matmul -- one utterance."""
    x = torch.arange(n_out, dtype=F64) + offset
    e = -prec[None, :] * (x[:, None] - c[None, :]) ** 2
    if bias is not None:
        e = e + bias[None, :]
    e = e.masked_fill(torch.arange(c.shape[0])[None, :] >= tx_b, float("-inf"))
    return torch.softmax(e, dim=-1) @ h, torch.logsumexp(e, dim=-1)


@pytest.mark.parametrize("make", [R.espnet_problem, R.mix_problem])
def test_reference_is_float64_autograd_of_the_composed_form(make):
    p = make(65, 33, 80, "f32")
    ref = R.evaluate(p)
    txs, tys = R.lengths(p)
    for b in range(4):
        if txs[b] == 0 or tys[b] == 0:
            assert not any(np.any(ref[k][b]) for k in R.OUTPUTS)
            continue
        t = {k: torch.tensor(p[k][b], dtype=F64, requires_grad=True) for k in ("h", "center", "prec")}
        bias = None if p["bias"] is None else torch.tensor(p["bias"][b], dtype=F64, requires_grad=True)
        y, lse = composed(t["h"], t["center"], t["prec"], bias, p["offset"], tys[b], txs[b])
        y.backward(torch.tensor(p["dy"][b, :tys[b]], dtype=F64))
        assert np.abs(ref["y"][b, :tys[b]] - y.detach().numpy()).max() < 1e-12
        assert np.abs(ref["lse"][b, :tys[b]] - lse.detach().numpy()).max() < 1e-11
        assert not ref["y"][b, tys[b]:].any() and not ref["lse"][b, tys[b]:].any()
        pairs = [("dh", t["h"].grad), ("dcenter", t["center"].grad), ("dprec", t["prec"].grad)]
        if bias is not None:
            pairs.append(("dbias", bias.grad))
        for name, g in pairs:
            g = g.numpy()
            assert np.abs(ref[name][b] - g).max() <= 1e-12 * max(np.abs(g).max(), 1.0), name
            assert not ref[name][b, txs[b]:].any(), name


def test_reference_through_durations_delta_and_sigma():
    """ESPnet's form from durations and delta, and Non-Attentive Tacotron's from durations and sigma:
    the chain rule over the reference's dcenter / dprec / dbias is torch's gradient."""
    rng = np.random.default_rng(0)
    tx, n_out, dim = 9, 30, 5
    d = rng.uniform(1, 5, size=tx)
    sig = rng.uniform(0.5, 2.0, size=tx)
    h, dy = rng.normal(size=(tx, dim)), rng.normal(size=(n_out, dim))
    for form in ("espnet", "nat"):
        dt, st, ht = (torch.tensor(v, dtype=F64, requires_grad=True) for v in (d, sig, h))
        c = torch.cumsum(dt, 0) - dt / 2
        if form == "espnet":
            prec, bias, offset = st, None, 0.0                 # a learned delta per phoneme
        else:
            prec, bias, offset = 1 / (2 * st ** 2), -torch.log(st), 1.0
        y, _ = composed(ht, c, prec, bias, offset, n_out, tx)
        y.backward(torch.tensor(dy))
        p = {"h": h[None], "dy": dy[None], "center": c.detach().numpy()[None], "prec": prec.detach().numpy()[None],
             "bias": None if bias is None else bias.detach().numpy()[None], "offset": offset, "q_len": None,
             "key_len": None, "dtype": "f32"}
        ref = R.evaluate(p)
        dc = ref["dcenter"][0]
        dd = np.cumsum(dc[::-1])[::-1] - dc / 2                # c_t = sum_{u <= t} d_u - d_t / 2
        assert np.abs(dd - dt.grad.numpy()).max() < 1e-11
        ds = ref["dprec"][0] if form == "espnet" else -ref["dprec"][0] / sig ** 3 - ref["dbias"][0] / sig
        assert np.abs(ds - st.grad.numpy()).max() < 1e-11
        assert np.abs(ref["dh"][0] - ht.grad.numpy()).max() < 1e-12


def test_bf16_rounding_helpers():
    x = np.random.default_rng(1).normal(size=1000) * 10.0 ** np.random.default_rng(2).integers(-3, 4, size=1000)
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16)
    assert np.array_equal(R.bf16_round(x), want.double().numpy())
    assert np.array_equal(R.bf16_bits(R.bf16_round(x)), want.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.bf16_from_bits(R.bf16_bits(R.bf16_round(x))), R.bf16_round(x))


def test_premises_of_the_exact_problems():
    assert np.exp(np.float32(-256.0)) == 0.0 and np.float32(np.exp(-256.0)) == 0.0     # one-hot in float32
    R.assert_uniform_premise()
    for shape in R.SHAPES + R.EDGE_SHAPES:
        n_out, tx, dim = shape
        for dtype in ("f32", "bf16"):
            p = R.selector_problem(*shape, dtype)
            txs, tys = R.lengths(p)
            assert txs == tys
            want = R.exact_expected(p)
            assert R.exact_outputs(p) == list(R.OUTPUTS), shape
            for b, n in enumerate(tys):
                assert np.array_equal(want["y"][b, :n], p["h"][b, :n]) and np.array_equal(want["dh"][b, :n], p["dy"][b, :n])
            assert not want["lse"].any() and not want["dcenter"].any() and not want["dprec"].any() and not want["dbias"].any()

            p = R.uniform_problem(*shape, dtype)
            txs, tys = R.lengths(p)
            assert all(t in (0,) + R.UNIFORM_TX for t in txs) and max(txs) == max(v for v in R.UNIFORM_TX if v <= tx)
            want, ref = R.exact_expected(p), R.evaluate(p)
            exact = R.exact_outputs(p)
            assert set(exact) >= {"y", "dh", "dcenter", "dbias"}, (shape, exact)
            assert "dprec" in exact or n_out > 5
            for k in exact:
                assert np.array_equal(want[k], ref[k]), (shape, k)       # the float64 values themselves
            for b in range(4):
                if txs[b] and tys[b]:
                    assert np.array_equal(want["y"][b, :tys[b]], np.broadcast_to(p["h"][b, :txs[b]].mean(axis=0), (tys[b], dim)))
            assert not want["dcenter"].any()
    # the largest shapes compare dprec through the bar: its float32 sum is order-dependent there
    assert "dprec" not in R.exact_outputs(R.uniform_problem(130, 129, 512, "f32"))


PROBLEMS = [(R.mix_problem, (65, 33, 80)), (R.mix_problem, (130, 129, 512)), (R.espnet_problem, (65, 33, 80))]
INVISIBLE = {R.espnet_problem: ("offset dropped", "bias ignored")}      # offset 0, no bias: nothing to get wrong


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("make,shape", PROBLEMS)
def test_the_bar_accepts_the_yardsticks_and_rejects_every_mutant(make, shape, dtype):
    p = make(*shape, dtype)
    ref, yard, sc = R.evaluate(p), R.yardstick(p), (R.scales(p), R.tiny(p))
    for y in yard:
        ratios, pads = R.judge(p, y, ref=ref, yard=yard, sc=sc)
        assert not pads and max(ratios.values()) <= 0.25 + 1e-12
    assert not R.rejected(p, ref, ref=ref, yard=yard, sc=sc)
    for name in R.MUTANTS:
        if name in INVISIBLE.get(make, ()):
            continue
        for confine in (False, True):
            assert R.rejected(p, R.mutant(p, name, confine), ref=ref, yard=yard, sc=sc), (name, confine)


def test_mutants_differ_only_inside_the_tile_when_confined():
    p = R.mix_problem(65, 33, 80, "f32")
    ref = R.evaluate(p)
    for name in R.MUTANTS:
        m = R.mutant(p, name, confine=True)
        assert R.confined_tile(65) == (32, 64) and R.confined_tile(33) == (0, 32)
        for k in ("y", "lse"):
            assert np.array_equal(m[k][:, :32], ref[k][:, :32]) and np.array_equal(m[k][:, 64:], ref[k][:, 64:])
        for k in ("dh", "dcenter", "dprec", "dbias"):
            assert np.array_equal(m[k][:, 32:], ref[k][:, 32:])


def test_padding_must_be_plus_zero():
    p = R.mix_problem(33, 5, 17, "f32")
    ref = R.evaluate(p)
    assert R.padding_faults(p, ref) == []
    bad = {k: v.copy() for k, v in ref.items()}
    bad["y"][1, -1, 0] = -0.0
    bad["dbias"][3, 0] = 1e-30
    assert sorted(R.padding_faults(p, bad)) == ["dbias", "y"]


@pytest.mark.parametrize("make", [R.espnet_problem, R.mix_problem])
def test_the_flush_to_zero_allowance_measured_on_the_float32_reference(make):
    """The float32 reference with every weight below 2^-126 flushed to zero, as the GPU has them: the
    flush raises its ratio on the rows that hold little but such weights (a row that holds nothing else
    loses its whole value, which no relative bar admits), and with the absolute allowance of FTZ times
    what the weights multiply it passes."""
    p = make(257, 37, 96, "f32")
    ref, yard, sc = R.evaluate(p), R.yardstick(p), (R.scales(p), R.tiny(p))
    flushed = R.evaluate(p, dt=np.float32, ftz=True)
    plain, _ = R.judge(p, flushed, ref=ref, yard=yard, sc=sc, ftz=False)
    with_allowance, pads = R.judge(p, flushed, ref=ref, yard=yard, sc=sc)
    print({k: (round(plain[k], 3), round(with_allowance[k], 3)) for k in plain})
    assert all(plain[k] >= with_allowance[k] for k in plain)
    assert not pads and max(with_allowance.values()) <= 1.0
    # the allowance is far below anything a mutant changes: the largest is this many float32 ulp of the row's scale
    assert (R.FTZ * sc[1]["dh"]).max() < 1e-30


THIRD = [(make, shape, dtype) for make in (R.espnet_problem, R.mix_problem)
         for shape in ((64, 64, 64), (65, 33, 80), (257, 37, 96), (130, 129, 512)) for dtype in ("f32", "bf16")]


def test_the_pooled_yardstick_measured_on_a_third_evaluation():
    """The issue's bar takes the yardstick's error row by row.  A yardstick is one draw (two in f32) of
    the rounding errors, and a row of dcenter, dprec or dbias is one number: on some rows the draw is
    tens of times smaller than on the neighbouring rows, and another evaluation of the same arithmetic
    misses 4 x that draw although it is exactly as accurate.  Here that other evaluation is numpy in
    the kernels' order (evaluate(tiled=True): online softmax over phoneme tiles, in bf16 the weights
    rounded relative to the running maximum; frames in blocks of 128) and, in float32, with the score
    rounded once as a fused multiply-add rounds it (fma=True): the two float32 yardsticks share the
    bits of e, so their errors on a row whose weights all sit at e = -27 are one draw, not two.
    judge() therefore counts the yardstick's error on a row as no less than its RMS error relative to
    scale over the utterance's rows.  Measured here on that evaluation (no kernel involved), worst
    ratio over the problems of THIRD, row by row / pooled:
        f32   y 0.75 / 0.69, lse 0.72 / 0.72, dh 8.27 / 0.61, dcenter 0.82 / 0.26, dprec 0.82 / 0.25, dbias 0.83 / 0.26
        bf16  y 0.25 / 0.25, lse 0.00 / 0.00, dh 0.25 / 0.25, dcenter 21.5 / 0.50, dprec 30.7 / 0.68, dbias 12.3 / 0.41
    The kernels' own worst ratios, which the GPU tests print against both bars, are the same figures:
    f32 dh 7.98 / 0.78, bf16 dcenter 21.5 / 0.50, dprec 30.7 / 0.68, dbias 12.3 / 0.61; every other
    output is below 1 row by row as well.
    The assertions below hold the measurement.  Every mutant is still rejected with the pooling
    (test_the_bar_accepts_the_yardsticks_and_rejects_every_mutant)."""
    worst = {False: {}, True: {}}
    for make, shape, dtype in THIRD:
        p = make(*shape, dtype)
        ref, yard, sc = R.evaluate(p), R.yardstick(p), (R.scales(p), R.tiny(p))
        third = R.evaluate(p, dt=np.float32, tiled=True, fma=True) if dtype == "f32" else R.evaluate(p, twin=True, tiled=True)
        for pool in (False, True):
            ratios, pads = R.judge(p, third, ref=ref, yard=yard, sc=sc, pool=pool)
            assert not pads
            for k, v in ratios.items():
                worst[pool][(dtype, k)] = max(worst[pool].get((dtype, k), 0.0), v)
    for dtype in ("f32", "bf16"):
        print(dtype, ", ".join(f"{k} {worst[False][(dtype, k)]:.3g} / {worst[True][(dtype, k)]:.3g}" for k in R.OUTPUTS))
    assert max(worst[True].values()) <= 1.0
    assert all(worst[False][("bf16", k)] > 10.0 for k in ("dcenter", "dprec", "dbias"))
    assert worst[False][("f32", "dh")] > 5.0
