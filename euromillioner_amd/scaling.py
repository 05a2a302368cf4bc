"""Per-group scaling of a model's logits (temperature / Platt scaling): statistics, Newton fit, apply, ``.cal`` file.

This module is the specification (numpy, no torch).  ``csrc/calibration_fit.hip`` (``ops.calibration_fit``) computes
the same statistics on device logits; both engines run the one Newton driver :func:`fit`.

A calibrator is four **float32** numbers ``a[0], a[1], b[0], b[1]``: a scale and a shift per output group (g = 0 is
outputs 0-49, g = 1 is outputs 50-61; columns 62-63 are pads and never read).  ``a[g]`` is finite and > 0; under the
softmax head ``b[g] = 0`` always (the shift cancels inside the group's softmax).  The calibrated logit is

    u = fl32(fl32(a[g] * z) + b[g])

two separately rounded float32 operations, no fused multiply-add: :func:`apply_np` and the kernel agree bit for bit.

For a row with logits ``z`` and target bits ``y`` let ``n_g = max(popcount of y in group g, 1)`` (the clamp of the
``loss`` of ``metrics.draw_metrics``).  The statistics of group g at ``(a, b)`` are the sums over rows of

===========  ===============================================  ====================================
             ``"softmax"``                                    ``"bce"``
===========  ===============================================  ====================================
``L``        ``lse_o(u_o) - a zy``, ``zy = sum y_o z_o / n``  ``sum softplus(u_o) - y_o u_o``
``g_a``      ``E_q[z] - zy``, ``q = softmax(u)``              ``sum (sigma(u_o) - y_o) z_o``
``g_b``      0                                                ``sum (sigma(u_o) - y_o)``
``h_aa``     ``sum q_o (z_o - E_q[z])^2``                     ``sum w_o z_o^2``, ``w = sigma (1 - sigma)``
``h_ab``     0                                                ``sum w_o z_o``
``h_bb``     0                                                ``sum w_o``
===========  ===============================================  ====================================

in the order ``L, g_a, g_b, h_aa, h_ab, h_bb`` (:data:`STATS`).  At ``a = 1, b = 0`` the per-row loss
(:func:`row_loss`) is the ``loss`` of ``draw_metrics``.  Both heads are convex in ``(a, b)``.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

NF, N_MAIN = 62, 50
LOSSES = ("softmax", "bce")
STATS = ("L", "g_a", "g_b", "h_aa", "h_ab", "h_bb")
A_MIN = 2.0 ** -20  # the fit keeps a at or above this
MAX_ITER, MAX_HALVINGS = 30, 20
CAL_VERSION = 1
_DRAW_BITS = np.uint64((1 << NF) - 1)


def check_loss(loss: str) -> str:
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {', '.join(LOSSES)}, got {loss!r}")
    return loss


def check_ab(a, b, loss: str) -> tuple[np.ndarray, np.ndarray]:
    """``(a, b)`` as float32 [2] arrays; ``ValueError`` unless a is finite and > 0, b is finite, and b is 0 under the
    softmax head."""
    check_loss(loss)
    try:
        a32, b32 = np.asarray(a, dtype=np.float32).reshape(-1), np.asarray(b, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError) as err:
        raise ValueError(f"a and b must be two numbers each ({err})") from err
    if a32.shape != (2,) or b32.shape != (2,):
        raise ValueError("a and b must be two numbers each (one per output group)")
    if not np.all(np.isfinite(a32)) or not np.all(a32 > 0):
        raise ValueError(f"the scales a must be finite and > 0, got {a32.tolist()}")
    if not np.all(np.isfinite(b32)):
        raise ValueError(f"the shifts b must be finite, got {b32.tolist()}")
    if loss == "softmax" and np.any(b32 != 0):
        raise ValueError("the shifts b must be 0 under the softmax head (a shift cancels inside the group)")
    return a32, b32


def _check_inputs(z, target_masks):
    z = np.asarray(z)
    if z.ndim != 2 or z.shape[1] < NF:
        raise ValueError(f"logits must be [rows, >= {NF}]")
    tm = np.asarray(target_masks)
    if tm.ndim != 1 or tm.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)) or len(tm) != len(z):
        raise ValueError("target_masks must be a 1-D uint64 / int64 array with one mask per row of logits")
    return z[:, :NF].astype(np.float32), tm.view(np.uint64) & _DRAW_BITS


def _bits(tm: np.ndarray) -> np.ndarray:
    return ((tm[:, None] >> np.arange(NF, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64)


def _u32(z32: np.ndarray, a: np.float32, b: np.float32) -> np.ndarray:
    """The calibrated logits of one group: float32, product and sum rounded separately."""
    return (np.float32(a) * z32).astype(np.float32) + np.float32(b)


def _group_n(yg: np.ndarray, g: int) -> np.ndarray:
    """n_g per row: the target bits of the group, at least 1 (not the nominal 5 / 2)."""
    return np.maximum(yg.sum(1), 1.0)


def _variance(q: np.ndarray, zg: np.ndarray, ez: np.ndarray) -> np.ndarray:
    """Per row ``sum q (z - E)^2``, centred on the known mean (never a difference of moments)."""
    return (q * (zg - ez[:, None]) ** 2).sum(1)


def apply_np(z, a, b) -> np.ndarray:
    """float32 [rows, 64]: ``u`` in columns 0-61, 0 in the pads."""
    a32, b32 = check_ab(a, b, "bce")
    z = np.asarray(z)
    if z.ndim != 2 or z.shape[1] < NF:
        raise ValueError(f"logits must be [rows, >= {NF}]")
    z32 = z[:, :NF].astype(np.float32)
    out = np.zeros((len(z32), 64), dtype=np.float32)
    out[:, :N_MAIN] = _u32(z32[:, :N_MAIN], a32[0], b32[0])
    out[:, N_MAIN:NF] = _u32(z32[:, N_MAIN:], a32[1], b32[1])
    return out


def stats_np(z, target_masks, loss: str, a=(1.0, 1.0), b=(0.0, 0.0)) -> np.ndarray:
    """float64 [2, 6]: the statistics (:data:`STATS`) of the rows of ``z`` [rows, >= 62] (read as float32), row r
    scored against ``target_masks[r]``.  ``u`` is formed in float32 as the definition says, everything after it in
    float64.  Argument errors are ``ValueError``, raised before anything is computed."""
    a32, b32 = check_ab(a, b, loss)
    z32, tm = _check_inputs(z, target_masks)
    y = _bits(tm)
    out = np.zeros((2, 6), dtype=np.float64)
    for g, sl in enumerate((slice(0, N_MAIN), slice(N_MAIN, NF))):
        zg, yg = z32[:, sl].astype(np.float64), y[:, sl]
        u = _u32(z32[:, sl], a32[g], b32[g]).astype(np.float64)
        if loss == "softmax":
            m = u.max(1, keepdims=True)
            e = np.exp(u - m)
            s = e.sum(1, keepdims=True)
            q = e / s
            zy = (yg * zg).sum(1) / _group_n(yg, g)
            ez = (q * zg).sum(1)
            out[g, 0] = float(((m[:, 0] + np.log(s[:, 0])) - float(a32[g]) * zy).sum())
            out[g, 1] = float((ez - zy).sum())
            out[g, 3] = float(_variance(q, zg, ez).sum())
        else:
            e = np.exp(-np.abs(u))
            sg = np.where(u >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
            w = e / (1.0 + e) ** 2
            out[g, 0] = float((np.maximum(u, 0.0) + np.log1p(e) - yg * u).sum())
            out[g, 1] = float(((sg - yg) * zg).sum())
            out[g, 2] = float((sg - yg).sum())
            out[g, 3] = float((w * zg * zg).sum())
            out[g, 4] = float((w * zg).sum())
            out[g, 5] = float(w.sum())
    return out


def row_loss(stats, rows: int, loss: str) -> float:
    """The per-row loss of ``draw_metrics`` from the two ``L`` sums: their sum over rows under softmax, over
    62 x rows under bce."""
    check_loss(loss)
    tot = float(stats[0][0]) + float(stats[1][0])
    return tot / (rows if loss == "softmax" else NF * rows)


def _newton_step(st: np.ndarray, loss: str):
    """The fp64 Newton step ``(da, db)`` of one group from its six statistics; None where the Hessian is not
    positive definite."""
    _, ga, gb, haa, hab, hbb = (float(v) for v in st)
    if loss == "softmax":
        if not haa > 0.0:
            return None
        return -ga / haa, 0.0
    det = haa * hbb - hab * hab
    if not (haa > 0.0 and hbb > 0.0 and det > 0.0):
        return None
    return -(hbb * ga - hab * gb) / det, -(haa * gb - hab * ga) / det


def fit(stats_fn, loss: str) -> dict:
    """The Newton driver both engines share.  ``stats_fn(a, b)`` takes float32 [2] arrays and returns the fp64 [2, 6]
    totals at that point.

    From ``a = 1, b = 0``, per iteration and per group: the fp64 Newton step (1 x 1 under softmax, 2 x 2 under bce),
    halved until the candidate's ``L`` is not larger than the current ``L`` (at most 20 halvings).  The candidate is
    the step rounded to float32 with ``a`` kept >= 2^-20.  A group stops (``converged``) when its rounded candidate
    equals its current point, and stops without converging when no halving lowers ``L``, when its Hessian is not
    positive definite, or after 30 iterations.  The groups are fitted independently but share the passes: one call
    serves both, and a group that has stopped keeps its point.

    Returns ``{"a", "b"`` (float32 [2]), ``"iterations", "converged"`` (per group), ``"L_before", "L_after"`` (fp64
    [2]), ``"passes"`` (calls of ``stats_fn``)}``."""
    check_loss(loss)
    a, b = np.ones(2, dtype=np.float32), np.zeros(2, dtype=np.float32)
    cur = np.array(stats_fn(a.copy(), b.copy()), dtype=np.float64)
    if cur.shape != (2, 6) or not np.all(np.isfinite(cur)):
        raise ValueError("the statistics must be a finite [2, 6] array")
    passes = 1
    before = cur[:, 0].copy()
    active, converged, iterations = [True, True], [False, False], [0, 0]
    for _ in range(MAX_ITER):
        steps = {}
        for g in (0, 1):
            if not active[g]:
                continue
            step = _newton_step(cur[g], loss)
            if step is None:
                active[g] = False
                converged[g] = cur[g, 1] == 0.0 and cur[g, 2] == 0.0
                continue
            steps[g] = step
            iterations[g] += 1
        if not steps:
            break
        scale = {g: 1.0 for g in steps}
        for _h in range(MAX_HALVINGS + 1):
            ca, cb = a.copy(), b.copy()
            for g in list(steps):
                ca[g] = np.float32(max(float(a[g]) + scale[g] * steps[g][0], A_MIN))
                cb[g] = np.float32(float(b[g]) + scale[g] * steps[g][1])
                if ca[g] == a[g] and cb[g] == b[g]:  # the step is below the float32 resolution of the point
                    active[g], converged[g] = False, True
                    del steps[g]
            if not steps:
                break
            st = np.array(stats_fn(ca.copy(), cb.copy()), dtype=np.float64)
            passes += 1
            for g in list(steps):
                if st[g, 0] <= cur[g, 0]:
                    a[g], b[g], cur[g] = ca[g], cb[g], st[g]
                    del steps[g]
                else:
                    scale[g] *= 0.5
        for g in steps:  # no halving lowered L
            active[g] = False
    return {"a": a, "b": b, "iterations": iterations, "converged": converged, "L_before": before,
            "L_after": cur[:, 0].copy(), "passes": passes}


def fit_np(z, target_masks, loss: str) -> dict:
    """:func:`fit` over :func:`stats_np` on host logits."""
    check_loss(loss)
    z32, tm = _check_inputs(z, target_masks)
    if len(z32) < 1:
        raise ValueError("fit needs at least one row")
    return fit(lambda a, b: stats_np(z32, tm, loss, a, b), loss)


class Calibrator:
    """The fitted ``(a, b)`` of one checkpoint, with the record of its fit.  ``record`` keys: ``model`` (checkpoint
    kind), ``lags``, ``first`` / ``last`` (the fitted sample range ``[first, last)``), ``rows``, ``iterations``,
    ``converged``, ``loss_before`` / ``loss_after`` (per row, on the fit rows) and ``checkpoint`` (base name)."""

    RECORD = ("model", "lags", "first", "last", "rows", "iterations", "converged", "loss_before", "loss_after",
              "checkpoint")

    def __init__(self, loss: str, a, b, record: dict | None = None):
        self.a, self.b = check_ab(a, b, loss)
        self.loss = loss
        self.record = dict(record or {})

    def apply_np(self, z) -> np.ndarray:
        return apply_np(z, self.a, self.b)

    def to_dict(self) -> dict:
        d = {"version": CAL_VERSION, "loss": self.loss,
             "a_hex": [float(v).hex() for v in self.a], "b_hex": [float(v).hex() for v in self.b],
             "a": [float(v) for v in self.a], "b": [float(v) for v in self.b]}
        d.update({k: self.record[k] for k in self.RECORD if k in self.record})
        return d

    def save(self, path: str) -> None:
        tmp = path + ".tmp"
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(self.to_dict(), f, indent=1)
            f.write("\n")
        os.replace(tmp, path)

    @classmethod
    def load(cls, path: str) -> "Calibrator":
        """Read a ``.cal`` file; a malformed one (not JSON, unknown version, wrong loss, values that are not finite
        float32 or not positive scales) is a ``ValueError``."""
        try:
            with open(path, encoding="utf-8") as f:
                d = json.load(f)
        except (json.JSONDecodeError, UnicodeDecodeError) as err:
            raise ValueError(f"{path}: not a calibrator file ({err})") from err
        if not isinstance(d, dict) or d.get("version") != CAL_VERSION:
            raise ValueError(f"{path}: calibrator version {d.get('version') if isinstance(d, dict) else None!r}, "
                             f"this build reads version {CAL_VERSION}")
        loss = d.get("loss")
        if loss not in LOSSES:
            raise ValueError(f"{path}: loss {loss!r} is none of {', '.join(LOSSES)}")
        vals = []
        for key in ("a_hex", "b_hex"):
            h = d.get(key)
            if not isinstance(h, list) or len(h) != 2 or not all(isinstance(s, str) for s in h):
                raise ValueError(f"{path}: {key} must be two float.hex strings")
            try:
                v = [float.fromhex(s) for s in h]
            except (ValueError, OverflowError) as err:
                raise ValueError(f"{path}: {key}: {err}") from err
            if not all(math.isfinite(x) and float(np.float32(x)) == x for x in v):
                raise ValueError(f"{path}: {key} must hold finite float32 values")
            vals.append(v)
        try:
            cal = cls(loss, vals[0], vals[1], {k: d[k] for k in cls.RECORD if k in d})
        except ValueError as err:
            raise ValueError(f"{path}: {err}") from err
        for key in ("lags", "first", "last", "rows"):
            v = cal.record.get(key)
            if v is not None and (not isinstance(v, int) or isinstance(v, bool) or v < 0):
                raise ValueError(f"{path}: {key} must be a non-negative integer")
        return cal
