"""The Adam reference (``_adam_ref.py``) checked before it judges ``csrc/adam.hip``: the slab sum against int64,
the fp64 step against ``torch.optim.Adam`` in float64, the derived bounds against an honest numpy fp32 evaluation
(accepted, worst ratio printed) and against planted mistakes (each rejected by the very checks the GPU tests use),
and the integer round-to-nearest-even against torch's cast.
"""
import numpy as np
import pytest
import torch

import _adam_ref as R

N_ELEMS = 200_000
STEPS = (1, 2, 3, 50)
SCALE = 1.0 / 3.0


def _hp(wd):
    return R.hp_f32(wd=wd)


# ---------------------------------------------------------------- slab sum

def _slab_kernel_f32(slabs, nslab, P, scale, mutate=None):
    """numpy stand-in for a slab-reducing kernel: fp32 sum of rows 0..nslab-1, then the scale."""
    rows = list(range(nslab))
    if mutate == "dropped":
        rows.remove(nslab // 2)
    elif mutate == "twice":
        rows.append(nslab // 3)
    elif mutate == "one_past":
        rows.append(nslab)
    acc = np.zeros(P, dtype=np.float32)
    for r in rows:
        acc = acc + slabs[r, :P]
    return acc * np.float32(scale)


@pytest.mark.parametrize("nslab,P,stride", [(1, 1, 1), (17, 100, 132), (257, 64, 68), (513, 128, 128)])
def test_slab_sum_matches_int64(nslab, P, stride):
    ints = R.int_slabs(nslab + 2, stride, seed=nslab)
    slabs = ints.copy()
    slabs[nslab:] = np.nan
    slabs[:, P:] = np.nan
    want = ints[:nslab, :P].astype(np.int64).sum(axis=0)
    for scale in (1.0, 2.0 ** -10, 4.0):
        got = R.slab_sum(slabs, nslab, P, scale)
        assert got.dtype == np.float64 and np.array_equal(got, want * scale)
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got)  # exact in fp32: equality is fair
    assert np.abs(ints).max() <= 4095 and np.abs(ints).min() >= 1


@pytest.mark.parametrize("mutate", [None, "dropped", "twice", "one_past"])
def test_slab_check_accepts_honest_rejects_planted(mutate):
    nslab, P, stride, scale = 241, 128, 132, 2.0 ** -10
    slabs = R.int_slabs(nslab + 2, stride, seed=3)
    slabs[nslab:] = np.nan
    slabs[:, P:] = np.nan
    got = _slab_kernel_f32(slabs, nslab, P, scale, mutate)
    assert R.slab_exact(got, slabs, nslab, P, scale) == (mutate is None)


def test_slab_float_bound_holds_for_fp32_sum():
    nslab, P = 257, 128
    rng = np.random.default_rng(5)
    slabs = rng.standard_normal((nslab, P)).astype(np.float32)
    got = _slab_kernel_f32(slabs, nslab, P, SCALE).astype(np.float64)
    ratio = np.abs(got - R.slab_sum(slabs, nslab, P, SCALE)) / (2 * R.slab_sum_bound(slabs, nslab, P, SCALE))
    print(f"sequential fp32 slab sum, nslab {nslab}: worst error / bound {ratio.max():.4f}")
    assert ratio.max() <= 1.0


# ---------------------------------------------------------------- Adam step

def test_bias_correction():
    for beta in (0.9, 0.999):
        b = float(np.float32(beta))
        for t in (1, 2, 3, 50, 1000):
            p = 1.0
            for _ in range(t):
                p *= b
            got = R.bias_correction(np.float32(beta), t)
            assert got.dtype == np.float32 and abs(float(got) - (1.0 - p)) <= 2.0 ** -24 * (1.0 - p)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_step_matches_torch_float64(wd):
    n = 4096
    hp = _hp(wd)
    lr, b1, b2, eps, wd64 = (float(x) for x in hp)
    scale = float(np.float32(SCALE))
    _, w0, _, _ = R.adam_inputs(n, 1, seed=11)
    w = w0.astype(np.float64)
    m, v = np.zeros(n), np.zeros(n)
    p = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd64)
    for t in range(1, 7):
        g = R.adam_inputs(n, 1, seed=100 + t)[0]
        p.grad = torch.tensor(g.astype(np.float64) * scale)
        opt.step()
        ref = R.adam_step(g, w, m, v, hp, t, SCALE, round_bc=False)
        # the float32-rounded bias corrections move the reference by less than a quarter of its own bound
        rounded = R.adam_step(g, w, m, v, hp, t, SCALE)
        assert np.all(np.abs(rounded.w - ref.w) <= 0.25 * rounded.tw)
        w, m, v = ref.w, ref.m, ref.v
        st = opt.state[p]
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("t", STEPS)
def test_honest_fp32_evaluation_is_accepted(t, wd):
    g, w, m, v = R.adam_inputs(N_ELEMS, t, seed=t)
    assert (g == 0).any() and (np.abs(g[g != 0]) < 1e-5).any()
    hp = _hp(wd)
    ref = R.adam_step(g, w, m, v, hp, t, SCALE)
    r = R.ratios(*R.adam_step_f32(g, w, m, v, hp, t, SCALE), ref)
    print(f"fp32 emulation t={t} wd={wd}: worst error / doubled bound w {r['w']:.3f} m {r['m']:.3f} v {r['v']:.3f}")
    assert max(r.values()) <= 0.5, r


ADAM_MUTATIONS = ["t_plus_1", "t_minus_1", "eps_in_sqrt", "no_wd", "scale_twice", "mv_swapped"]


@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("mutate", ADAM_MUTATIONS)
def test_planted_adam_mistakes_are_rejected(mutate, t):
    g, w, m, v = R.adam_inputs(N_ELEMS, t, seed=t)
    hp = _hp(0.01)
    ref = R.adam_step(g, w, m, v, hp, t, SCALE)
    with np.errstate(all="ignore"):
        got = R.adam_step_f32(g, w, m, v, hp, t, SCALE, mutate=mutate)
    r = R.ratios(*got, ref)
    print(f"{mutate} t={t}: worst error / doubled bound w {r['w']:.3g} m {r['m']:.3g} v {r['v']:.3g}")
    assert not R.accepted(*got, ref), r


@pytest.mark.parametrize("t", [1, 2, 3])
def test_exp_log_bias_correction_is_rejected(t):
    """``1 - exp2(t * log2(beta))`` in fp32.  At t = 1 numpy's correctly rounded ``exp2(log2(beta))`` returns
    ``beta`` itself for both betas, so the form is exact there and no check can (or should) tell it apart; that is
    asserted as such.  From t = 2 on the cancellation costs ~1e-5 of ``bc2`` and the bound rejects it."""
    g, w, m, v = R.adam_inputs(N_ELEMS, t, seed=t)
    hp = _hp(0.0)
    ref = R.adam_step(g, w, m, v, hp, t, SCALE)
    got = R.adam_step_f32(g, w, m, v, hp, t, SCALE, mutate="bc_exp_log")
    r = R.ratios(*got, ref)
    print(f"bc_exp_log t={t}: worst error / doubled bound w {r['w']:.3g}")
    if t == 1:
        f = np.float32
        for beta in hp[1:3]:
            assert f(1) - np.exp2(f(1) * np.log2(beta, dtype=f), dtype=f) == R.bias_correction(beta, 1)
        honest = R.adam_step_f32(g, w, m, v, hp, t, SCALE)
        assert all(np.array_equal(a, b) for a, b in zip(got, honest))
    else:
        assert not R.accepted(*got, ref), r


def test_ratios_treat_nan_and_zero_bounds():
    g, w, m, v = R.adam_inputs(64, 1, seed=0)
    g[:] = 0
    hp = _hp(0.0)
    ref = R.adam_step(g, w, m, v, hp, 1)
    assert np.all(ref.tm == 0) and np.all(ref.tv == 0) and np.array_equal(ref.w, w.astype(np.float64))
    assert R.accepted(w, m, v, ref)
    bad = m.copy()
    bad[3] = 1e-30
    assert not R.accepted(w, bad, v, ref)  # a zero bound admits only the exact value
    bad = w.copy()
    bad[5] = np.nan
    assert not R.accepted(bad, m, v, ref)


# ---------------------------------------------------------------- bf16

def test_bf16_rne_bits_matches_torch_on_directed_vector():
    bits = R.cast_directed_bits()
    x = bits.view(np.float32)
    want = torch.from_numpy(x.copy()).bfloat16().view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_rne_bits(x)
    nan = np.isnan(x)
    assert nan.sum() == 8 and np.array_equal(R.bf16_is_nan(got), nan) and np.array_equal(R.bf16_is_nan(want), nan)
    assert np.array_equal(got[~nan], want[~nan])
    assert R.bf16_bits_match(want, x) and R.bf16_bits_match(got.view(np.int16), x)
    pin = {0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80, 0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F807FFF: 0x3F80,
           0x3F808001: 0x3F81, 0x00000001: 0x0000, 0x80000001: 0x8000, 0x00018000: 0x0002, 0x3FFF8000: 0x4000}
    for src, dst in pin.items():
        assert int(got[list(bits).index(src)]) == dst, hex(src)


def test_bf16_rne_bits_matches_torch_on_random_patterns():
    rng = np.random.default_rng(9)
    bits = rng.integers(0, 2 ** 32, size=100_000, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    want = torch.from_numpy(x.copy()).bfloat16().view(torch.int16).numpy()
    assert R.bf16_bits_match(want, x)


def test_truncating_cast_and_stale_shadow_are_rejected():
    x = R.cast_directed_bits().view(np.float32)
    assert not R.bf16_bits_match(R.bf16_trunc_bits(x), x)
    g, w, m, v = R.adam_inputs(4096, 1, seed=2)
    w1, _, _ = R.adam_step_f32(g, w, m, v, _hp(0.0), 1)
    assert R.bf16_bits_match(R.bf16_rne_bits(w1), w1)
    assert not R.bf16_bits_match(R.bf16_rne_bits(w), w1)  # shadow taken from the pre-update weights
    assert not R.bf16_bits_match(R.bf16_trunc_bits(w1), w1)
