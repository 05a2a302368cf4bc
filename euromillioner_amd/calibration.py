"""Calibration of a model's probabilities: reliability table, Brier score, expected calibration error.

This module is the specification (numpy, no torch).  ``csrc/calibration.hip`` (``ops.calibration``) computes the
same totals on device logits; on the GPU the logits never leave the device.

Per row of logits ``z[0..61]`` (columns 62-63 are pads and never read), a target mask ``tm`` (bit o = output o was
drawn) and a head kind (the ``loss`` strings of ``draw_metrics``):

===========  =================================================  ==============================
             ``"softmax"``                                      ``"bce"``
===========  =================================================  ==============================
binned x     ``z - logsumexp(z over its group)``                ``z``
predicted q  ``exp(x)``                                         ``sigmoid(z)``
target t     ``y / k``, nominal k = 5 (main) / 2 (stars)        ``y``
===========  =================================================  ==============================

The groups are outputs 0-49 (main numbers) and 50-61 (stars).  ``y / k`` is the value at which the grouped
cross-entropy the models train on is minimal, so a perfectly calibrated softmax head has ``mean_q == hits / (k
count)`` in every bin.

Bins: up to 15 strictly ascending probability edges in (0, 1) give at most 16 bins.  :func:`edges_x` converts them
to x-space as **float32** (``logit(p)`` under bce, ``log(p)`` under softmax); that float32 table is what both engines
compare against, and ``bin = number of edges e with float32(x) >= e``.

Totals (:func:`calibration_np`): per (group, bin) ``counts`` and ``hits`` (elements with ``y = 1``) as int64 [2, 16]
and ``sum_q`` as float64 [2, 16]; per group ``brier = sum (q - t)^2`` as float64 [2].  :func:`report` turns totals
into the reliability table, the Brier score per row and the expected calibration error.
"""
from __future__ import annotations

import math

import numpy as np

NF, N_MAIN = 62, 50
GROUPS = ("main", "stars")
K_NOMINAL = (5, 2)
MAX_EDGES, N_BINS = 15, 16
LOSSES = ("softmax", "bce")
DEFAULT_EDGES = (0.005, 0.01, 0.02, 0.03, 0.05, 0.075, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5, 0.7, 0.9, 0.99)
_DRAW_BITS = np.uint64((1 << NF) - 1)


def check_edges(edges) -> tuple:
    """The probability edges as a tuple of floats; ``ValueError`` unless they are at most 15, finite, inside (0, 1)
    and strictly ascending."""
    try:
        e = tuple(float(v) for v in edges)
    except (TypeError, ValueError) as err:
        raise ValueError(f"edges must be a sequence of numbers ({err})") from err
    if len(e) > MAX_EDGES:
        raise ValueError(f"at most {MAX_EDGES} edges ({N_BINS} bins), got {len(e)}")
    for v in e:
        if not math.isfinite(v) or not 0.0 < v < 1.0:
            raise ValueError(f"edge {v!r}: edges are probabilities inside (0, 1)")
    if any(b <= a for a, b in zip(e, e[1:])):
        raise ValueError("edges must be strictly ascending")
    return e


def check_loss(loss: str) -> str:
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {', '.join(LOSSES)}, got {loss!r}")
    return loss


def edges_x(edges, loss: str) -> np.ndarray:
    """float32 [len(edges)]: the edges in x-space, ``logit(p)`` under bce and ``log(p)`` under softmax, computed in
    fp64 and rounded once.  Edges that collapse onto one float32 value are refused."""
    check_loss(loss)
    p = np.asarray(check_edges(edges), dtype=np.float64)
    x = (np.log(p) - np.log1p(-p) if loss == "bce" else np.log(p)).astype(np.float32)
    if np.any(x[1:] <= x[:-1]):
        raise ValueError("edges must stay strictly ascending as float32 x-space values")
    return x


def _check_inputs(z, target_masks):
    z = np.asarray(z)
    if z.ndim != 2 or z.shape[1] < NF:
        raise ValueError(f"logits must be [rows, >= {NF}]")
    tm = np.asarray(target_masks)
    if tm.ndim != 1 or tm.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)) or len(tm) != len(z):
        raise ValueError("target_masks must be a 1-D uint64 / int64 array with one mask per row of logits")
    return z[:, :NF].astype(np.float64), tm.view(np.uint64) & _DRAW_BITS


def _group_lse(z: np.ndarray) -> np.ndarray:
    m = z.max(1, keepdims=True)
    return m + np.log(np.exp(z - m).sum(1, keepdims=True))


def x_q_np(z, loss: str) -> tuple[np.ndarray, np.ndarray]:
    """(x, q) float64 [rows, 62] of logits [rows, >= 62]."""
    check_loss(loss)
    z = np.asarray(z)[:, :NF].astype(np.float64)
    if loss == "bce":
        with np.errstate(over="ignore"):
            return z, 1.0 / (1.0 + np.exp(-z))
    x = np.concatenate([z[:, :N_MAIN] - _group_lse(z[:, :N_MAIN]), z[:, N_MAIN:] - _group_lse(z[:, N_MAIN:])], axis=1)
    return x, np.exp(x)


def _bin_of(x: np.ndarray, ex: np.ndarray) -> np.ndarray:
    """int64, shape of x: the number of float32 edges e with float32(x) >= e."""
    return (x.astype(np.float32)[..., None] >= ex).sum(-1)


def _target(y: np.ndarray, g: int, loss: str) -> np.ndarray:
    """The value q is held against: y under bce, y / k (nominal k of group g) under softmax."""
    return y / K_NOMINAL[g] if loss == "softmax" else y.astype(np.float64)


def bins_np(z, loss: str, edges=DEFAULT_EDGES) -> np.ndarray:
    """uint8 [rows, 62]: the bin of every element."""
    ex = edges_x(edges, loss)
    return _bin_of(x_q_np(z, loss)[0], ex).astype(np.uint8)


def calibration_np(z, target_masks, loss: str, edges=DEFAULT_EDGES) -> dict:
    """Totals ``{"counts", "hits", "sum_q", "brier"}`` over the rows of ``z`` [rows, >= 62], row r scored against
    ``target_masks[r]``.  Argument errors are ``ValueError``, raised before anything is computed."""
    ex = edges_x(edges, loss)
    z, tm = _check_inputs(z, target_masks)
    x, q = x_q_np(z, loss)
    b = _bin_of(x, ex)
    y = ((tm[:, None] >> np.arange(NF, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)
    out = {"counts": np.zeros((2, N_BINS), dtype=np.int64), "hits": np.zeros((2, N_BINS), dtype=np.int64),
           "sum_q": np.zeros((2, N_BINS), dtype=np.float64), "brier": np.zeros(2, dtype=np.float64)}
    for g, sl in enumerate((slice(0, N_MAIN), slice(N_MAIN, NF))):
        bg, yg, qg = b[:, sl].reshape(-1), y[:, sl].reshape(-1), q[:, sl].reshape(-1)
        out["counts"][g] = np.bincount(bg, minlength=N_BINS)
        out["hits"][g] = np.bincount(bg, weights=yg, minlength=N_BINS).astype(np.int64)
        out["sum_q"][g] = np.bincount(bg, weights=qg, minlength=N_BINS)
        out["brier"][g] = float(((qg - _target(yg, g, loss)) ** 2).sum())
    return out


def add_totals(a: dict | None, b: dict) -> dict:
    """Sum of two totals (``a`` may be None): the integers in int64, the sums in float64."""
    if a is None:
        return {k: np.array(v, dtype=np.int64 if k in ("counts", "hits") else np.float64) for k, v in b.items()
                if k in ("counts", "hits", "sum_q", "brier")}
    return {k: a[k] + np.asarray(b[k], dtype=a[k].dtype) for k in a}


def report(totals: dict, rows: int, loss: str, edges=None) -> dict:
    """The calibration report of ``rows`` rows: per group the reliability table (one entry per bin: ``mean_q``, the
    observed value ``hits / count``, divided by k under softmax, and ``count``; empty bins carry None), ``brier``
    per row and ``ece = sum_b count_b / N |mean_q_b - observed_b|``."""
    check_loss(loss)
    rows = int(rows)
    if rows < 1:
        raise ValueError("report needs at least one row")
    out: dict = {"rows": rows, "loss": loss}
    if edges is not None:
        out["edges"] = [float(v) for v in edges]
    for g, name in enumerate(GROUPS):
        cnt, hits = np.asarray(totals["counts"][g], dtype=np.int64), np.asarray(totals["hits"][g], dtype=np.int64)
        sq = np.asarray(totals["sum_q"][g], dtype=np.float64)
        k = K_NOMINAL[g] if loss == "softmax" else 1
        n = int(cnt.sum())
        table, ece = [], 0.0
        for b in range(N_BINS):
            c = int(cnt[b])
            if c == 0:
                table.append({"bin": b, "mean_q": None, "observed": None, "count": 0})
                continue
            mq, ob = float(sq[b]) / c, float(hits[b]) / (c * k)
            ece += c / n * abs(mq - ob)
            table.append({"bin": b, "mean_q": mq, "observed": ob, "count": c})
        out[name] = {"bins": table, "count": n, "hits": int(hits.sum()), "brier": float(totals["brier"][g]) / rows,
                     "ece": ece}
    return out


def bin_label(b: int, edges) -> str:
    """``[lo, hi)`` of bin b in probability space."""
    e = (0.0,) + tuple(edges) + (1.0,)
    return f"[{e[b]:g}, {e[b + 1]:g}" + ("]" if b + 1 == len(e) - 1 else ")")


def format_report(rep: dict, edges) -> str:
    """The reliability table as text: per group one line per non-empty bin."""
    lines = []
    for name in GROUPS:
        g = rep[name]
        lines.append(f"{name}: brier/row {g['brier']:.6f}  ece {g['ece']:.6f}  ({g['count']} elements, {g['hits']} drawn)")
        lines.append(f"  {'bin':<16}{'mean_q':>12}{'observed':>12}{'count':>12}")
        for r in g["bins"]:
            if r["count"]:
                lines.append(f"  {bin_label(r['bin'], edges):<16}{r['mean_q']:>12.6f}{r['observed']:>12.6f}{r['count']:>12}")
    return "\n".join(lines)
