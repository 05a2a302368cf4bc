"""fp64 reference of the scaling statistics (``euromillioner_amd/scaling.py``, ``csrc/calibration_fit.hip``) and
the fp32 error budget of each of them.  numpy only, plain loops over the outputs, written from the table of
definitions and sharing no code with ``scaling.py``: it judges the numpy specification (``test_scaling_cpu.py``) and
the HIP kernel (``test_scaling_gpu.py``).

Definitions
-----------
Groups: g = 0 is outputs 0-49, g = 1 is outputs 50-61.  ``u_o = fl32(fl32(a[g] z_o) + b[g])`` (float32, part of the
definition); everything after it is fp64 here.  With target bits ``y`` and ``n = max(popcount y, 1)``, a row adds

* softmax: ``m = max u``, ``d_o = u_o - m``, ``S = sum exp d_o``, ``q_o = exp(d_o) / S``, ``E = sum q_o z_o``,
  ``zy = sum y_o z_o / n``; ``L = m + log S - a zy``, ``g_a = E - zy``, ``h_aa = sum q_o (z_o - E)^2``;
* bce: ``e_o = exp(-|u_o|)``, ``sigma_o = 1 / (1 + e_o)`` or ``e_o / (1 + e_o)`` by the sign of ``u_o``,
  ``w_o = e_o / (1 + e_o)^2``; ``L = sum max(u_o, 0) + log(1 + e_o) - y_o u_o``, ``g_a = sum (sigma_o - y_o) z_o``,
  ``g_b = sum (sigma_o - y_o)``, ``h_aa = sum w_o z_o^2``, ``h_ab = sum w_o z_o``, ``h_bb = sum w_o``.

Every statistic comes back as ``S`` (the value) and ``A``: the sum of the magnitudes of everything that is added or
subtracted in forming it, each weighted by how strongly the statistic depends on it.  A term that carries an
exponential is counted ``c`` times, ``c_o = 1 + |d_o|`` (softmax) or ``1 + |u_o|`` (bce), because the exponent itself
is a rounded fp32 number whose absolute error is ``u |exponent|`` and turns into a relative error of the exponential.
Per row and group ``A`` is

=========  ==========================================================================================
softmax
``L``      ``sum q_o c_o`` (the terms of ``S``, relative to ``S``: what ``log S`` sees) ``+ |m| + |log S|``
           ``+ a sum y_o |z_o| / n`` (``|a zy|`` and the terms ``zy`` is formed from)
``g_a``    ``sum q_o c_o (|z_o| + |E|)`` (numerator and, through ``1 / S``, denominator) ``+ sum y_o |z_o| / n``
``h_aa``   ``sum q_o c_o ((z_o - E)^2 + h_aa)``
bce
``L``      ``sum max(u_o, 0) + (1 + log(1 + e_o)) + y_o |u_o|`` (the 1 is the one that ``1 + e_o`` adds)
``g_a``    ``sum (sigma_o c_o + y_o) |z_o|``      ``g_b``: ``sum sigma_o c_o + y_o``
``h_aa``   ``sum w_o c_o z_o^2``      ``h_ab``: ``sum w_o c_o |z_o|``      ``h_bb``: ``sum w_o c_o``
=========  ==========================================================================================

The budget ``K u A``
--------------------
``u = 2^-24`` is the unit roundoff of fp32.  The kernel evaluates the formulas above in fp32 with ``__expf`` (a
product with log2(e), rounded, then the hardware 2^x, 1 ulp = 2u), ``__logf`` (the hardware log2, 1 ulp = 2u, then a
rounded product with ln 2), the hardware reciprocal (1 ulp = 2u) and plain products and sums (u each; an fma only
removes a rounding).  To first order the errors add:

* an exponential: the exponent ``d = u_o - m`` rounds once (``u |d|`` absolute; under bce ``-|u_o|`` is exact), its
  product with log2(e) rounds once (another ``u |d|`` on the exponent), the 2^x is 2u relative:
  at most ``(2 |d| + 2) u <= 2 c u`` relative.  Arguments are <= 0, so the results are <= 1 and nothing overflows; a
  result below 2^-126 is flushed to 0.  The budget is relative, so like that of ``tests/_adam_ref.py`` it needs
  sums that stay clear of fp32's underflow: a row whose logits are all at +-120 has an ``h_aa`` of 1e-45, made of
  terms fp32 cannot hold.  :func:`logits` therefore places such rows so that every 256-row block (and B = 1) also
  holds ordinary rows, whose terms are of order 1.
* what multiplies it: ``z_o - E`` (u), its square (2u + u), the product with the exponential (u); under bce
  ``r = 1 / (1 + e)`` (u for the sum, 2u for the reciprocal) enters ``w = (e r) r`` twice (6u) with two products
  (2u), then ``w z`` and ``(w z) z`` (2u); ``sigma`` takes ``r`` once, a product, the difference ``sigma - y`` and
  the product with ``z`` (6u): at most 10u.
* the sum: a lane adds at most 50 terms of a group in order, the wave butterfly adds 6 times, the block 2 times:
  every term passes at most 50 + 6 + 2 = 58 additions, 58u.
* the softmax denominator: ``S`` carries the errors of its exponentials and 49 additions,
  ``(2 sum q_o c_o + 49) u <= 51 u sum q_o c_o`` relative; the reciprocal and the product with it add 3u.  It enters
  ``E`` and ``h_aa`` relative to their own size and ``log S`` absolutely: that is the second part of their ``A``.
* the rest of ``L``: ``log S`` rounds to ``3u |log S|``; ``m + log S``, the product ``a zy`` and the final difference
  round once each; ``zy`` is a sum of at most 50 terms and one correctly rounded division (51u).  Under bce
  ``log(1 + e)``: the sum ``1 + e`` rounds to u (1 + e) and the logarithm passes that on absolutely (<= 2u), the
  error of ``e`` enters as ``e / (1 + e)`` times its relative error (<= 2u), ``__logf`` adds ``3u log(1 + e)``: at
  most ``4u (1 + log(1 + e))``.

The largest total is that of an ``h_aa`` term, ``(2 c + 10 + 58) u <= 70 c u``, next to ``54 u`` on the
denominator part; the ``L`` terms stay below ``64 u`` each.  ``K = 72`` covers every statistic.  The tests allow
**2 x** the budget: the factor covers the second-order terms this first-order analysis drops (the doubled convention
of ``tests/_adam_ref.py``).  ``K`` was fixed from this derivation before the kernel ran.
"""
from __future__ import annotations

import functools

import numpy as np

U32 = 2.0 ** -24
K = 72.0
FACTOR = 2.0
GROUPS = ((0, 50), (50, 62))
STATS = ("L", "g_a", "g_b", "h_aa", "h_ab", "h_bb")


def bits(masks) -> np.ndarray:
    """[rows] uint64 / int64 masks -> [rows, 62] {0, 1} float64."""
    m = np.asarray(masks).view(np.uint64)
    return np.stack([((m >> np.uint64(o)) & np.uint64(1)).astype(np.float64) for o in range(62)], axis=1)


def calibrated(z32: np.ndarray, a, b) -> np.ndarray:
    """float32 u of one column: product and sum rounded separately."""
    p = np.multiply(np.float32(a), z32, dtype=np.float32)
    return np.add(p, np.float32(b), dtype=np.float32)


def reference_rows(z, Y, loss: str, a, b) -> tuple[np.ndarray, np.ndarray]:
    """(S, A), each float64 [rows, 2, 6]: per row and group the six statistics and their magnitude sums.
    ``z`` [rows, >= 62] is read as float32, ``Y`` [rows, 62] holds the target bits."""
    z32 = np.asarray(z)[:, :62].astype(np.float32)
    Y = np.asarray(Y, dtype=np.float64)
    rows = len(z32)
    S, A = np.zeros((rows, 2, 6)), np.zeros((rows, 2, 6))
    for g, (lo, hi) in enumerate(GROUPS):
        ag, bg = np.float32(a[g]), np.float32(b[g])
        zc = [z32[:, o].astype(np.float64) for o in range(lo, hi)]
        uc = [calibrated(z32[:, o], ag, bg).astype(np.float64) for o in range(lo, hi)]
        yc = [Y[:, o] for o in range(lo, hi)]
        if loss == "softmax":
            m = uc[0].copy()
            for u in uc[1:]:
                m = np.maximum(m, u)
            ssum, n, ysum, yabs = np.zeros(rows), np.zeros(rows), np.zeros(rows), np.zeros(rows)
            for zo, u, y in zip(zc, uc, yc):
                ssum += np.exp(u - m)
                n += y
                ysum += y * zo
                yabs += y * np.abs(zo)
            n = np.maximum(n, 1.0)
            zy, yabs = ysum / n, yabs / n
            E, qc = np.zeros(rows), np.zeros(rows)
            for zo, u in zip(zc, uc):
                q = np.exp(u - m) / ssum
                E += q * zo
                qc += q * (1.0 + np.abs(u - m))
            h, a_g, a_h = np.zeros(rows), np.zeros(rows), np.zeros(rows)
            for zo, u in zip(zc, uc):
                q = np.exp(u - m) / ssum
                c = 1.0 + np.abs(u - m)
                h += q * (zo - E) ** 2
                a_g += q * c * (np.abs(zo) + np.abs(E))
                a_h += q * c * (zo - E) ** 2
            af = float(ag)
            S[:, g, 0] = m + np.log(ssum) - af * zy
            A[:, g, 0] = qc + np.abs(m) + np.abs(np.log(ssum)) + af * yabs
            S[:, g, 1] = E - zy
            A[:, g, 1] = a_g + yabs
            S[:, g, 3] = h
            A[:, g, 3] = a_h + h * qc
        elif loss == "bce":
            for zo, u, y in zip(zc, uc, yc):
                e = np.exp(-np.abs(u))
                sg = np.where(u >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
                w = e / (1.0 + e) ** 2
                c = 1.0 + np.abs(u)
                S[:, g, 0] += np.maximum(u, 0.0) + np.log1p(e) - y * u
                A[:, g, 0] += np.maximum(u, 0.0) + 1.0 + np.log1p(e) + y * np.abs(u)
                S[:, g, 1] += (sg - y) * zo
                A[:, g, 1] += (sg * c + y) * np.abs(zo)
                S[:, g, 2] += sg - y
                A[:, g, 2] += sg * c + y
                S[:, g, 3] += w * zo * zo
                A[:, g, 3] += w * c * zo * zo
                S[:, g, 4] += w * zo
                A[:, g, 4] += w * c * np.abs(zo)
                S[:, g, 5] += w
                A[:, g, 5] += w * c
        else:
            raise ValueError(loss)
    return S, A


def reference(z, Y, loss: str, a=(1.0, 1.0), b=(0.0, 0.0)) -> tuple[np.ndarray, np.ndarray]:
    """(S, A), each float64 [2, 6]: the totals over the rows."""
    S, A = reference_rows(z, Y, loss, a, b)
    return S.sum(0), A.sum(0)


def budget(A) -> np.ndarray:
    """The fp32 budget ``K u A`` (the tests allow ``FACTOR`` times it)."""
    return K * U32 * np.asarray(A, dtype=np.float64)


def within(got, S, A, factor: float = FACTOR) -> np.ndarray:
    """Elementwise ``|got - S| <= factor K u A`` (a NaN is outside)."""
    return np.abs(np.asarray(got, dtype=np.float64) - S) <= factor * budget(A)


# ------------------------------------------------------------------------------------------------ test inputs
def masks(n: int, seed: int = 7) -> np.ndarray:
    """[n] int64 draw masks: 5 mains and 2 stars per draw; every 11th draw has no main, every 13th no star, every
    17th 3 mains and 1 star, every 7th carries bits 62-63 (which no consumer may read)."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        m = 0
        few = i % 17 == 4
        if i % 11 != 3:
            for o in rng.choice(50, 3 if few else 5, replace=False):
                m |= 1 << int(o)
        if i % 13 != 5:
            for o in rng.choice(12, 1 if few else 2, replace=False):
                m |= 1 << (50 + int(o))
        if i % 7 == 2:
            m |= 3 << 62
        out[i] = m
    return out.view(np.int64)


def logits(rows: int, seed: int = 1) -> np.ndarray:
    """float32 [rows, 64]: N(0, 2^2) logits, every 5th row (3, 8, ..: never row 0, 256 or 512, which can be alone in
    a block) with a fifth of its logits at +-120, NaN in the pads."""
    rng = np.random.default_rng(100 + seed)
    z = (2.0 * rng.standard_normal((rows, 64))).astype(np.float32)
    hot = np.arange(rows) % 5 == 3
    spikes = rng.random((rows, 64)) < 0.2
    sign = np.where(rng.random((rows, 64)) < 0.5, -120.0, 120.0).astype(np.float32)
    z = np.where(hot[:, None] & spikes, sign, z)
    z[:, 62:] = np.nan
    return z


POINTS = {"softmax": (((1.0, 1.0), (0.0, 0.0)), ((0.25, 0.25), (0.0, 0.0)), ((4.0, 4.0), (0.0, 0.0))),
          "bce": (((1.0, 1.0), (0.0, 0.0)), ((0.25, 0.25), (3.0, 3.0)), ((4.0, 4.0), (-3.0, -3.0)))}


def planted(loss: str, rows: int = 4096, seed: int = 3, a=2.0, b=-1.0):
    """The planted fit case: float32 [rows, 64] N(0, 1.5^2) logits (pads 0) and [rows] int64 target masks sampled
    from the model ``softmax(a z)`` (one bit per group) or ``sigma(a z + b)`` (independent bits)."""
    rng = np.random.default_rng(1000 + seed)
    z = np.zeros((rows, 64), dtype=np.float32)
    z[:, :62] = (1.5 * rng.standard_normal((rows, 62))).astype(np.float32)
    tm = np.zeros(rows, dtype=np.uint64)
    z64 = z[:, :62].astype(np.float64)
    if loss == "softmax":
        for lo, hi in GROUPS:
            x = a * z64[:, lo:hi]
            p = np.exp(x - x.max(1, keepdims=True))
            cdf = np.cumsum(p / p.sum(1, keepdims=True), axis=1)
            pick = np.minimum((rng.random(rows)[:, None] > cdf).sum(1), hi - lo - 1)
            tm |= np.uint64(1) << (pick + lo).astype(np.uint64)
    else:
        y = rng.random((rows, 62)) < 1.0 / (1.0 + np.exp(-(a * z64 + b)))
        for o in range(62):
            tm |= y[:, o].astype(np.uint64) << np.uint64(o)
    return z, tm.view(np.int64)


def distance(fit_a, fit_b, true_a, true_b, H6) -> float:
    """``sqrt(d^T H d)`` of one group: d = fitted - planted parameters, H from the statistics ``h_aa, h_ab, h_bb``."""
    da, db = float(fit_a) - true_a, float(fit_b) - true_b
    return float(np.sqrt(H6[3] * da * da + 2.0 * H6[4] * da * db + H6[5] * db * db))


def kernel_order_f32(z, Y, loss: str, a, b) -> np.ndarray:
    """float32 [blocks, 2, 6]: the kernel's formulas in honest numpy float32 (every operation rounded, numpy's exp and
    log) and in the kernel's summation order: a lane (row) adds its elements in order, the 64 lanes of a wave go
    through the xor butterfly 32, 16, .. 1, the four waves of a 256-row block add as (w0 + w1) + (w2 + w3)."""
    f = np.float32
    z32 = np.asarray(z)[:, :62].astype(f)
    Y = np.asarray(Y) > 0.5
    rows = len(z32)
    nb = (rows + 255) // 256
    lane = np.zeros((nb * 256, 2, 6), dtype=f)
    with np.errstate(over="ignore", under="ignore"):
        for g, (lo, hi) in enumerate(GROUPS):
            ag, bg = f(a[g]), f(b[g])
            zc = [z32[:, o] for o in range(lo, hi)]
            uc = [calibrated(zo, ag, bg) for zo in zc]
            yc = [Y[:, o] for o in range(lo, hi)]
            zero = np.zeros(rows, dtype=f)
            if loss == "softmax":
                m = uc[0].copy()
                for u in uc[1:]:
                    m = np.maximum(m, u)
                S, T, ys, n = zero.copy(), zero.copy(), zero.copy(), zero.copy()
                for zo, u, y in zip(zc, uc, yc):
                    e = np.exp(u - m)
                    S = S + e
                    T = T + e * zo
                    ys = ys + np.where(y, zo, f(0))
                    n = n + y.astype(f)
                zy = ys / np.maximum(n, f(1))
                r = f(1) / S
                E = T * r
                V = zero.copy()
                for zo, u in zip(zc, uc):
                    e = np.exp(u - m)
                    d = zo - E
                    V = V + e * (d * d)
                lane[:rows, g, 0] = (m + np.log(S)) - ag * zy
                lane[:rows, g, 1] = E - zy
                lane[:rows, g, 3] = V * r
            else:
                acc = [zero.copy() for _ in range(6)]
                for zo, u, y in zip(zc, uc, yc):
                    e = np.exp(-np.abs(u))
                    r = f(1) / (f(1) + e)
                    er = e * r
                    sg = np.where(u >= 0, r, er)
                    w = er * r
                    acc[0] = acc[0] + ((np.maximum(u, f(0)) + np.log(f(1) + e)) - np.where(y, u, f(0)))
                    d = sg - y.astype(f)
                    acc[1] = acc[1] + d * zo
                    acc[2] = acc[2] + d
                    wz = w * zo
                    acc[3] = acc[3] + wz * zo
                    acc[4] = acc[4] + wz
                    acc[5] = acc[5] + w
                for k in range(6):
                    lane[:rows, g, k] = acc[k]
    assert lane.dtype == f
    v = lane.reshape(nb, 4, 64, 2, 6)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, idx ^ o]
    w = v[:, :, 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


# ------------------------------------------------------------------------------------------------ shared cases
BS = (1, 63, 64, 65, 255, 256, 257, 513)  # lane, wave and block edges, partial last blocks
N_MASKS = 700


@functools.lru_cache(maxsize=None)
def inputs() -> tuple[np.ndarray, np.ndarray]:
    """(logits float32 [513, 64], masks int64 [700]) of every statistics test; read-only."""
    z, m = logits(513), masks(N_MASKS)
    z.setflags(write=False)
    m.setflags(write=False)
    return z, m


def sample_index(B: int, seed: int) -> np.ndarray:
    """int32 [B] sample indices with repeats, each leaving a next draw."""
    return np.random.default_rng(500 + seed).integers(0, N_MASKS - 1, size=B).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case_reference(loss: str, point: int, B: int, offset: int = 0, sidx_seed: int | None = None):
    """(S, A) float64 [B, 2, 6] of the first B rows of :func:`inputs` at ``POINTS[loss][point]``, row s scored against
    ``masks[idx + 1]`` with ``idx = sample_index(B, sidx_seed)[s]`` or ``offset + s``.  Computed once per case."""
    z, m = inputs()
    idx = sample_index(B, sidx_seed).astype(np.int64) if sidx_seed is not None else offset + np.arange(B)
    a, b = POINTS[loss][point]
    S, A = reference_rows(z[:B], bits(m[idx + 1]), loss, a, b)
    S.setflags(write=False)
    A.setflags(write=False)
    return S, A


def block_sums(rows: np.ndarray) -> np.ndarray:
    """[rows, 2, 6] -> [blocks, 2, 6]: the sums over the 256-row blocks."""
    nb = (len(rows) + 255) // 256
    return np.stack([rows[256 * k:256 * k + 256].sum(0) for k in range(nb)])
