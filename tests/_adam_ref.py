"""fp64 reference and derived error bounds for ``csrc/adam.hip`` (K6): the slab sum, one Adam step, the
bias correction and the fp32 -> bf16 cast.  numpy only: no GPU and no torch kernel takes part, so the file can
judge the HIP kernels (``test_adam_kernels_gpu.py``) and is itself checked on the CPU (``test_adam_ref_cpu.py``).

The Adam bound
--------------
``u = 2^-24`` is the unit roundoff of fp32 (round to nearest).  The kernels evaluate, in fp32 and in this order,

    gs = g * scale                     ge = gs + wd * w
    m' = b1 * m + (1 - b1) * ge        v' = b2 * v + ((1 - b2) * ge) * ge
    D  = sqrt(v' / bc2) + eps          U  = lr * (m' / bc1) / D            w' = w - U

with ``bc = float32(1 - beta^t)`` (``beta^t`` in fp64).  Division and square root are correctly rounded.  Every
operation contributes a relative error of at most ``u``; to first order the errors add, each scaled by the
sensitivity of the result to the perturbed operand:

* ``ge``: the product ``g * scale``, the product ``wd * w`` and the sum round once each.  The sum's rounding is
  relative to ``|ge| <= |gs| + |wd w|``, each product's to itself, so ``tg = 3u (|gs| + |wd w|)`` (one ``u`` to
  spare).
* ``m'``: ``1 - b1`` rounds once (it scales the second term only), two products, one sum, i.e. at most ``4u`` on
  ``|b1 m| + |(1 - b1) ge|``; the inherited error of ``ge`` enters times ``1 - b1``:
  ``tm = 4u (|b1 m| + |(1 - b1) ge|) + (1 - b1) tg``.
* ``v'``: all terms are non-negative, so the roundings (``1 - b2``, three products, one sum) are relative to
  ``v'`` itself, ``5u v'``; ``d(ge^2) = 2 |ge| tg`` enters times ``1 - b2``:
  ``tv = 5u v' + 2 (1 - b2) |ge| tg``.
* ``U``: with ``s = sqrt(v' / bc2)``, the quotient ``v' / bc2``, the root, the sum ``s + eps``, the quotient
  ``m' / bc1``, the product with ``lr`` and the final quotient round once each (6u); the float32 rounding of
  ``bc1`` and ``bc2`` against the exact ``1 - beta^t`` is covered by the remaining ``2u``: ``8u |U|``.  ``m'``
  enters linearly, ``dU/dm' = lr / (bc1 D)``.  ``v'`` enters through ``s``: ``ds/s = dv' / (2 v')`` and
  ``dU/U = -(s / D) ds/s``, so the term is ``|U| (s / D) tv / (2 v')``, and 0 where ``v' = 0`` (then ``ge = 0``
  and ``tv = 0``: the kernel's ``v'`` is exactly 0 as well).
  ``tU = 8u |U| + lr / (bc1 D) tm + |U| (s / D) tv / (2 v')``.
* ``w'``: one subtraction, ``tw = u |w'| + tU``.

The tests allow **2 x** each bound: the factor covers the second-order terms this first-order analysis drops.
Contracting a product and a sum into one FMA only removes a rounding.  The bounds are relative, so the inputs
must stay clear of subnormals; :func:`adam_inputs` does.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

U32 = 2.0 ** -24  # unit roundoff of fp32
HP = (1e-3, 0.9, 0.999, 1e-8, 0.0)  # (lr, beta1, beta2, eps, weight_decay)
FACTOR = 2.0  # the tests allow FACTOR x each derived bound


def hp_f32(lr=HP[0], b1=HP[1], b2=HP[2], eps=HP[3], wd=HP[4]) -> np.ndarray:
    return np.array([lr, b1, b2, eps, wd], dtype=np.float32)


def slab_sum(slabs, nslab: int, P: int, scale) -> np.ndarray:
    """fp64 sum over rows ``0..nslab-1`` of columns ``0..P-1``, times ``float32(scale)``."""
    s = np.asarray(slabs)
    if s.ndim != 2 or nslab < 1 or nslab > s.shape[0] or P < 1 or P > s.shape[1]:
        raise ValueError("slabs must be [>= nslab, >= P]")
    return s[:nslab, :P].astype(np.float64).sum(axis=0) * float(np.float32(scale))


def slab_exact(got, slabs, nslab: int, P: int, scale) -> bool:
    """``got[:P]`` equals :func:`slab_sum` element for element (integer slabs, power-of-two scale)."""
    got = np.asarray(got)
    return got.shape == (P,) and bool(np.array_equal(got.astype(np.float64), slab_sum(slabs, nslab, P, scale)))


def int_slabs(rows: int, cols: int, seed: int) -> np.ndarray:
    """fp32 integers in [-4095, 4095], nowhere zero: with a power-of-two scale every summation order of up to
    4096 of them is exact in fp32 (|sum| < 2^24)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 4096, size=(rows, cols)) * rng.choice([-1, 1], size=(rows, cols))
    return a.astype(np.float32)


def slab_sum_bound(slabs, nslab: int, P: int, scale) -> np.ndarray:
    """Standard gamma_n bound of an fp32 sum of ``nslab`` terms in any order, times one more rounding for the
    scale: ``(nslab + 1) u |scale| sum |x|`` per column (the tests allow 2 x)."""
    a = np.abs(np.asarray(slabs)[:nslab, :P].astype(np.float64)).sum(axis=0)
    return (nslab + 1) * U32 * abs(float(np.float32(scale))) * a


def bias_correction(beta_f32, t: int) -> np.float32:
    """``float32(1 - float64(beta_f32) ** t)``"""
    return np.float32(1.0 - float(np.float32(beta_f32)) ** int(t))


class AdamRef(NamedTuple):
    w: np.ndarray
    m: np.ndarray
    v: np.ndarray
    tw: np.ndarray
    tm: np.ndarray
    tv: np.ndarray


def adam_step(g, w, m, v, hp, t: int, scale=1.0, round_bc: bool = True) -> AdamRef:
    """One torch.optim.Adam step (L2 weight decay folded into the gradient) in fp64 from the given operands and
    the float32-rounded ``hp`` and ``scale``, with the per-element first-order bounds of the module docstring.
    ``round_bc=False`` keeps the bias corrections in fp64 (torch.optim.Adam in float64 does)."""
    g, w, m, v = (np.asarray(x, dtype=np.float64) for x in (g, w, m, v))
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in hp)
    scale = float(np.float32(scale))
    if round_bc:
        bc1, bc2 = float(bias_correction(b1, t)), float(bias_correction(b2, t))
    else:
        bc1, bc2 = 1.0 - b1 ** int(t), 1.0 - b2 ** int(t)
    u = U32
    gs = g * scale
    ge = gs + wd * w
    tg = 3 * u * (np.abs(gs) + np.abs(wd * w))
    m1 = b1 * m + (1 - b1) * ge
    tm = 4 * u * (np.abs(b1 * m) + np.abs((1 - b1) * ge)) + (1 - b1) * tg
    v1 = b2 * v + (1 - b2) * ge * ge
    tv = 5 * u * v1 + 2 * (1 - b2) * np.abs(ge) * tg
    s = np.sqrt(v1 / bc2)
    D = s + eps
    upd = lr * (m1 / bc1) / D
    with np.errstate(divide="ignore", invalid="ignore"):
        via_v = np.where(v1 > 0, np.abs(upd) * (s / D) * tv / (2 * v1), 0.0)
    tU = 8 * u * np.abs(upd) + lr / (bc1 * D) * tm + via_v
    w1 = w - upd
    tw = u * np.abs(w1) + tU
    return AdamRef(w1, m1, v1, tw, tm, tv)


def ratios(got_w, got_m, got_v, ref: AdamRef, where=None) -> dict:
    """Worst ``|got - ref| / (FACTOR * bound)`` of each output (0 / 0 counts as 0, x / 0 as inf, a NaN or inf in
    ``got`` as inf).  A result is accepted when every ratio is <= 1."""
    out = {}
    for name, got, want, tol in (("w", got_w, ref.w, ref.tw), ("m", got_m, ref.m, ref.tm), ("v", got_v, ref.v, ref.tv)):
        got = np.asarray(got, dtype=np.float64)
        err = np.abs(got - want)
        err = np.where(np.isfinite(got), err, np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / (FACTOR * tol))
        if where is not None:
            r = r[where]
        out[name] = float(r.max()) if r.size else 0.0
    return out


def accepted(got_w, got_m, got_v, ref: AdamRef, where=None) -> bool:
    return all(r <= 1.0 for r in ratios(got_w, got_m, got_v, ref, where).values())


def adam_inputs(n: int, t: int, seed: int, zero_share: float = 1 / 16):
    """fp32 ``(g, w, m, v)`` of the Adam cases: ``|g|`` log-uniform in [1e-6, 1e3] with random sign and a share
    of exact zeros, ``w ~ N(0, 1)``; ``m = v = 0`` at ``t = 1``, else ``m ~ N(0, 0.1)`` and ``v ~ U(0, 0.1)``.
    Nothing is subnormal (``v`` is kept >= 1e-12), so the relative bounds hold; step 1 with tiny ``|g|`` is where a
    misplaced ``eps`` shows."""
    rng = np.random.default_rng(seed)
    g = 10.0 ** rng.uniform(-6.0, 3.0, n) * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < zero_share] = 0.0
    w = rng.standard_normal(n)
    if t <= 1:
        m, v = np.zeros(n), np.zeros(n)
    else:
        m = 0.1 * rng.standard_normal(n)
        v = np.maximum(rng.uniform(0.0, 0.1, n), 1e-12)
    return tuple(x.astype(np.float32) for x in (g, w, m, v))


def adam_step_f32(g, w, m, v, hp, t: int, scale=1.0, mutate: str | None = None):
    """numpy fp32 evaluation of the kernels' formula, operation by operation (the honest emulation), or with one
    planted mistake (``mutate``).  Returns fp32 ``(w', m', v')``."""
    f = np.float32
    g, w, m, v = (np.asarray(x, dtype=f) for x in (g, w, m, v))
    lr, b1, b2, eps, wd = (f(x) for x in hp)
    scale = f(scale)
    one = f(1.0)
    tt = {"t_plus_1": t + 1, "t_minus_1": t - 1}.get(mutate, t)
    if mutate == "bc_exp_log":  # 1 - exp2(t * log2(beta)) in fp32
        bc1 = one - np.exp2(f(t) * np.log2(b1, dtype=f), dtype=f)
        bc2 = one - np.exp2(f(t) * np.log2(b2, dtype=f), dtype=f)
    else:
        bc1, bc2 = bias_correction(b1, tt), bias_correction(b2, tt)
    gs = g * scale
    if mutate == "scale_twice":
        gs = gs * scale
    ge = gs if mutate == "no_wd" else gs + wd * w
    m1 = b1 * m + (one - b1) * ge
    v1 = b2 * v + ((one - b2) * ge) * ge
    if mutate == "eps_in_sqrt":
        D = np.sqrt(v1 / bc2 + eps)
    else:
        D = np.sqrt(v1 / bc2) + eps
    w1 = w - lr * (m1 / bc1) / D
    assert w1.dtype == f and m1.dtype == f and v1.dtype == f
    if mutate == "mv_swapped":
        m1, v1 = v1, m1
    return w1, m1, v1


def bf16_rne_bits(x_f32) -> np.ndarray:
    """fp32 -> bf16 bit patterns (uint16) by round-to-nearest-even in integer arithmetic on the bit pattern.
    NaN stays NaN (quieted, sign kept); the largest finite fp32 rounds to inf."""
    b = np.ascontiguousarray(np.asarray(x_f32, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (b >> 16) | 0x40, r)
    return r.astype(np.uint16)


def bf16_trunc_bits(x_f32) -> np.ndarray:
    """The planted mistake: truncation instead of RNE."""
    b = np.ascontiguousarray(np.asarray(x_f32, dtype=np.float32)).view(np.uint32)
    return (b >> 16).astype(np.uint16)


def bf16_is_nan(bits) -> np.ndarray:
    return (np.asarray(bits).view(np.uint16) & 0x7FFF) > 0x7F80


def bf16_bits_match(got_bits, x_f32) -> bool:
    """``got_bits`` (uint16 / int16 patterns) equals :func:`bf16_rne_bits` of ``x_f32``; a NaN matches any NaN."""
    got = np.asarray(got_bits).view(np.uint16)
    want = bf16_rne_bits(x_f32)
    nan = bf16_is_nan(want)
    return bool(np.array_equal(bf16_is_nan(got), nan) and np.array_equal(got[~nan], want[~nan]))


def cast_directed_bits() -> np.ndarray:
    """uint32 patterns of the directed cast vector: zeros, subnormals, inf, NaNs, the overflow-to-inf edge, ties
    under an even and an odd kept mantissa, ties +- 1 ulp, and the negatives of all of them."""
    pos = [
        0x00000000,  # +0
        0x00000001,  # smallest subnormal -> 0
        0x00008000,  # subnormal tie under an even (zero) kept mantissa -> 0
        0x00008001,  # just above it -> bf16 0x0001
        0x00018000,  # subnormal tie under an odd kept mantissa -> 0x0002
        0x007FFFFF,  # largest subnormal -> smallest normal
        0x00800000,  # smallest normal
        0x7F800000,  # inf
        0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA00000,  # NaNs (quiet, signalling, all ones)
        0x7F7FFFFF,  # largest finite -> inf
        0x7F7F8000,  # tie at the top binade under an odd mantissa -> inf
        0x7F7F7FFF,  # just below it -> largest finite bf16
        0x3F800000,  # 1.0
        0x3F808000, 0x3F807FFF, 0x3F808001,  # tie under an even kept mantissa, and -+ 1 ulp
        0x3F818000, 0x3F817FFF, 0x3F818001,  # tie under an odd kept mantissa, and -+ 1 ulp
        0x3FFF8000,  # tie under an all-ones mantissa: carries into the exponent
        0x40490FDB, 0x42F6E979, 0x3EAAAAAB,  # pi, 123.456, 1/3
    ]
    a = np.array(pos, dtype=np.uint32)
    return np.concatenate([a, a | np.uint32(0x80000000)])
