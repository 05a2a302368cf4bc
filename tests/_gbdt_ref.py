"""A plain fp64 reference of the GBDT watch-list metrics and of ``predict``, computed from fitted trees.

Numpy only; nothing here calls the oracle's routing helpers.  The tests fit a model, hand its trees and cuts
to :func:`margins_by_round`, and compare every round of every watch set with :func:`metric` inside
:func:`budget`.

Margins.  :func:`margins_by_round` bins X with the cuts (bin = number of cuts <= x, the rule of
``apply_bins``), walks the heap-numbered trees on the bins (right iff ``bin > sbin``, stop at ``status != 1``)
and replays the engines' accumulation exactly: ``m = float32(m + float32(leaf))`` once per round and task,
tree ``k`` belonging to task ``k % T``.  The result is float32 ``[R, n, T]``: the engines' margins bit for bit
if their kernels are right.

Metrics.  :func:`metric` takes those float32 margins and evaluates the definitions of
``euromillioner_amd/metrics.py`` in float64 (clip to [1e-16, 1 - 1e-16], rmse's root after the mean,
first-maximum arg-max).

Budgets.  :func:`budget` is the largest ``|engine - reference|`` allowed, computed from the reference's own
values only.  Error model: the engine evaluates the sigmoid in float32, within 4 ulp of the true value, so
for p in [1/2, 1) (spacing 2^-24) ``|dp| <= 2^-22``, and by symmetry the same holds for 1 - p when p < 1/2; a
float32 softmax probability over T classes is within (T + 4) 2^-24 relative; the result is stored as a
float32 (relative 2^-23 allowed).

* ``rmse`` (squared error): 2^-23 ref -- double arithmetic on identical float32 values on both sides.
* ``error`` / ``merror``: the COUNT must be equal, ``round(dev * count) == ref_count`` (exact while
  count < 2^22, asserted by :func:`check_preconditions`), and no element may sit in the ambiguous band: a
  non-zero logistic margin with |m| < 2^-20 (float32 p rounds to 1/2 there), or, for ``merror``, a non-zero gap
  below 2^-20 between the two largest class margins (a float32 softmax may tie them).  Squared error compares
  m > 0.5 exactly in float32, so m == 0.5 is simply "not above" and there is no band.
* ``logloss``: mean over elements of ``2^-21 + (1 - y) 2^-22 / (1 - p)`` for p >= 1/2 and
  ``2^-21 + y 2^-22 / p`` for p < 1/2 (first order in dp; valid while max |margin| <= 8, i.e.
  min(p, 1 - p) >= 3e-4), plus 2^-23 ref.
* ``mlogloss``: (T + 4) 2^-23 per row plus 2^-23 ref; the label's probability must be above 1e-6.

The band counts and the bounds on margins, probabilities and counts are preconditions
(:func:`check_preconditions`), not tolerances.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LOGISTIC = ("reg:logistic", "binary:logistic")
MULTI = ("multi:softprob", "multi:softmax")
COUNT_METRICS = ("error", "merror")
TRAIN = "<train_history>"  # key of the train-metric column in the refs of compare_history
MAX_ABS_MARGIN = 8.0
MIN_LABEL_PROB = 1e-6
MAX_COUNT = 1 << 22
BAND = 2.0 ** -20


# ----------------------------------------------------------------------------- margins
def bin_features(X, cuts) -> np.ndarray:
    """bin[r, f] = number of cuts of feature f that are <= X[r, f]."""
    X = np.asarray(X, np.float64)
    out = np.zeros(X.shape, dtype=np.int64)
    for f, c in enumerate(cuts):
        c = np.asarray(c, np.float64)
        if c.size:
            out[:, f] = (X[:, f, None] >= c[None, :]).sum(axis=1)
    return out


def leaf_values(trees, bins: np.ndarray, k: int) -> np.ndarray:
    """float32 leaf of tree k for every row of ``bins`` (heap walk: right iff bin > sbin)."""
    n = bins.shape[0]
    node = np.zeros(n, dtype=np.int64)
    rows = np.arange(n)
    for _ in range(trees.status.shape[1]):
        split = trees.status[k, node] == 1
        if not split.any():
            break
        nd = node[split]
        right = bins[rows[split], trees.feat[k, nd]] > trees.sbin[k, nd]
        node[split] = 2 * nd + 1 + right
    return np.asarray(trees.leaf[k, node], dtype=np.float32)


def margins_by_round(trees, cuts, n_tasks: int, base_margin: float, X) -> np.ndarray:
    """float32 [R, n, T]: the margins after each round, accumulated as the engines accumulate them."""
    bins = bin_features(X, cuts)
    T = int(n_tasks)
    K = trees.status.shape[0]
    assert K % T == 0
    R = K // T
    m = np.full((bins.shape[0], T), np.float32(base_margin), dtype=np.float32)
    out = np.empty((R,) + m.shape, dtype=np.float32)
    for r in range(R):
        for t in range(T):
            m[:, t] = (m[:, t] + leaf_values(trees, bins, r * T + t)).astype(np.float32)
        out[r] = m
    return out


def predict_range(trees, cuts, n_tasks: int, X, k0: int, k1: int):
    """fp64 sum, per (row, task), of the leaves of the trees k in [k0, k1) with k % T == task, the sum of their
    absolute values and the number of trees added: (sum [n, T], abs_sum [n, T], trees_per_task [T])."""
    bins = bin_features(X, cuts)
    T = int(n_tasks)
    s = np.zeros((bins.shape[0], T), dtype=np.float64)
    a = np.zeros_like(s)
    cnt = np.zeros(T, dtype=np.int64)
    for k in range(k0, k1):
        lv = leaf_values(trees, bins, k).astype(np.float64)
        s[:, k % T] += lv
        a[:, k % T] += np.abs(lv)
        cnt[k % T] += 1
    return s, a, cnt


# ----------------------------------------------------------------------------- metrics
def _labels(Y, n: int) -> np.ndarray:
    """class ids [n] from class ids or a one-hot matrix."""
    Y = np.asarray(Y)
    if Y.ndim == 2 and Y.shape[1] > 1:
        return np.argmax(Y, axis=1).astype(np.int64)
    return Y.reshape(n).astype(np.int64)


def _sigmoid64(m: np.ndarray) -> np.ndarray:
    return 1.0 / (1.0 + np.exp(-m))


def _softmax64(m: np.ndarray) -> np.ndarray:
    e = np.exp(m - m.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _prep(objective: str, Y, m32):
    m32 = np.asarray(m32)
    assert m32.dtype == np.float32 and m32.ndim == 2
    m = m32.astype(np.float64)
    if objective in MULTI:
        return m, _labels(Y, m.shape[0])
    y = np.asarray(Y, np.float64).reshape(m.shape[0], -1)
    assert y.shape == m.shape
    return m, y


def count_of(name: str, m32) -> int:
    """number of terms of the mean: rows for the multi-class metrics, elements otherwise."""
    m32 = np.asarray(m32)
    return int(m32.shape[0] if name in ("mlogloss", "merror") else m32.size)


def error_count(objective: str, name: str, Y, m32) -> int:
    m, y = _prep(objective, Y, m32)
    if name == "merror":
        return int(np.sum(np.argmax(m, axis=1) != y))  # first maximum
    assert name == "error"
    above = (m > 0.0) if objective in LOGISTIC else (m > 0.5)  # p > 0.5
    return int(np.sum(above.astype(np.float64) != y))


def metric(objective: str, name: str, Y, m32) -> float:
    """The eval metric of float32 margins [n, T] in float64."""
    m, y = _prep(objective, Y, m32)
    if name in COUNT_METRICS:
        return error_count(objective, name, Y, m32) / count_of(name, m32)
    if name == "mlogloss":
        p = _softmax64(m)
        return float(-np.mean(np.log(np.maximum(p[np.arange(len(p)), y], 1e-16))))
    p = _sigmoid64(m) if objective in LOGISTIC else m
    if name == "rmse":
        return float(np.sqrt(np.mean((y - p) ** 2)))
    assert name == "logloss"
    p = np.clip(p, 1e-16, 1.0 - 1e-16)
    return float(-np.mean(y * np.log(p) + (1.0 - y) * np.log(1.0 - p)))


def ambiguous(objective: str, name: str, m32) -> int:
    """elements (rows for merror) a float32 engine may legitimately classify either way."""
    m = np.asarray(m32).astype(np.float64)
    if name == "error" and objective in LOGISTIC:
        return int(np.sum((m != 0.0) & (np.abs(m) < BAND)))
    if name == "merror":
        top = np.sort(m, axis=1)[:, -2:]
        gap = top[:, 1] - top[:, 0]
        return int(np.sum((gap != 0.0) & (gap < BAND)))
    return 0


def budget(objective: str, name: str, Y, m32) -> float:
    """Largest |engine - reference| of this metric on these margins (see the module docstring); for the count
    metrics half a count, the value distance that ``round(dev * count) == ref_count`` amounts to."""
    m, y = _prep(objective, Y, m32)
    ref = metric(objective, name, Y, m32)
    if name in COUNT_METRICS:
        return 0.5 / count_of(name, m32)
    if name == "rmse":
        assert objective == "reg:squarederror"
        return 2.0 ** -23 * abs(ref)
    if name == "mlogloss":
        return (m.shape[1] + 4) * 2.0 ** -23 + 2.0 ** -23 * abs(ref)
    assert name == "logloss" and objective in LOGISTIC
    p = _sigmoid64(m)
    hi = 2.0 ** -21 + (1.0 - y) * 2.0 ** -22 / (1.0 - p)
    lo = 2.0 ** -21 + y * 2.0 ** -22 / p
    return float(np.mean(np.where(p >= 0.5, hi, lo))) + 2.0 ** -23 * abs(ref)


def check_preconditions(objective: str, name: str, Y, m32) -> None:
    """The conditions under which :func:`budget` is a bound (assertions on the reference's own inputs)."""
    m, y = _prep(objective, Y, m32)
    assert np.isfinite(m).all()
    assert count_of(name, m32) < MAX_COUNT, "count metrics are exact only below 2^22 terms"
    assert ambiguous(objective, name, m32) == 0, "margins inside the ambiguous band"
    if name == "logloss":
        assert np.abs(m).max() <= MAX_ABS_MARGIN, float(np.abs(m).max())
    if name == "mlogloss":
        pl = _softmax64(m)[np.arange(len(m)), y]
        assert pl.min() > MIN_LABEL_PROB, float(pl.min())


# ----------------------------------------------------------------------------- comparison
@dataclass(frozen=True)
class Ref:
    value: float
    budget: float
    count: int
    errors: int | None  # the exact count of the count metrics, None otherwise


def reference(objective: str, name: str, Y, margins) -> list[Ref]:
    """One Ref per round from float32 margins [R, n, T]; the preconditions are asserted on every round."""
    out = []
    for m32 in margins:
        check_preconditions(objective, name, Y, m32)
        out.append(Ref(metric(objective, name, Y, m32), budget(objective, name, Y, m32), count_of(name, m32),
                       error_count(objective, name, Y, m32) if name in COUNT_METRICS else None))
    return out


def _ok(dev: float, ref: Ref) -> bool:
    if not np.isfinite(dev):
        return False
    if ref.errors is not None:
        return int(round(dev * ref.count)) == ref.errors
    return abs(dev - ref.value) <= ref.budget


def compare_history(history, train_history, refs) -> list[tuple]:
    """Every round of every set of ``refs`` (set name -> [Ref per round]; ``TRAIN`` -> the refs of
    ``train_history``) against ``history`` (list of {"round", set: value}) and ``train_history`` (list of
    floats, or None when ``refs`` has no ``TRAIN``).  Returns the violations (round, set, dev, ref, budget);
    a missing round, set or value is a violation with dev = nan."""
    bad = []
    for name, rr in refs.items():
        for r, ref in enumerate(rr):
            if name == TRAIN:
                dev = float(train_history[r]) if train_history is not None and r < len(train_history) else np.nan
            else:
                rec = history[r] if r < len(history) else {}
                dev = float(rec[name]) if name in rec and rec.get("round") == r else np.nan
            if not _ok(dev, ref):
                bad.append((r, name, dev, ref.value, ref.budget))
        got = len(history) if name != TRAIN else (-1 if train_history is None else len(train_history))
        if got != len(rr):  # rounds the reference does not have
            bad.append((len(rr), name, float("nan"), float("nan"), 0.0))
    return bad


def worst_ratio(history, train_history, refs) -> float:
    """max |dev - ref| / budget over the non-count entries of ``refs`` (how much room the budgets leave)."""
    w = 0.0
    for name, rr in refs.items():
        for r, ref in enumerate(rr):
            if ref.errors is not None or ref.budget <= 0:
                continue
            dev = train_history[r] if name == TRAIN else history[r][name]
            w = max(w, abs(float(dev) - ref.value) / ref.budget)
    return w


def same_within(a: float, b: float, rel: float = 1e-6) -> bool:
    """The project's rule for two groupings of the same sum: |a - b| <= rel * max(1, |b|)."""
    return abs(a - b) <= rel * max(1.0, abs(b))
