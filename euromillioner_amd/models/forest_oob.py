"""Out-of-bag (OOB) evaluation and feature importances of the random forest: the numpy specification.

A bagged forest carries its own held-out estimate: row ``i`` is out of bag for tree ``t`` when its
bootstrap weight is 0, and here that weight is ``poisson_weights(seed, global tree id, N)[i]`` -- a counter
hash, so the in-bag sets are never stored: they are recomputed exactly from three integers, at predict
time, and the fit does not change.  The HIP engine (``csrc/forest.hip`` K11-OOB, ``ops/forest.py``) follows
the definitions here operation for operation:

* ``count[i]``: the trees ``t`` with ``poisson_weights(seed, tree_start + t, N)[i] == 0``;
* ``proba[i]``: the fp32 sum, in ascending tree order, of those trees' leaf vectors, divided (fp32) by
  ``count[i]``; all zero where ``count[i] == 0``;
* the score covers the rows with ``count > 0``.  Picks: stable top-5 of outputs 0..49 and top-2 of 50..61
  on the fp32 probabilities (the earlier index wins a tie: ``csrc/draw_topk.h``); ``acc`` / ``exact`` /
  ``trivial_acc`` as ``losses.draw_metrics_torch``; ``brier``: row mean of the fp32 sum over j (ascending)
  of ``(p_j - y_j)^2``; ``logloss``: row mean of the 62-term mean BCE, ``-log(p_j)`` or ``-log(1 - p_j)``
  with ``p`` clamped in fp32 to ``[1e-7f, 1 - 1e-7f]`` and the complement ``1 - p`` formed in fp32 too
  (``log(1 - p)`` is ill-conditioned at the clamp's floor: in fp64 it would be another metric there);
  the per-row fp32 values are added in fp64.
"""
from __future__ import annotations

import numpy as np

# the integer totals of a score, in the order of em_rf_oob_metrics' per-block words 0..7
TOTAL_KEYS = ("rows", "hits_main", "hits_star", "exact", "mismatch_bits", "target_bits", "min_trees", "trees_sum",
              "brier_sum", "logloss_sum")
P_LO, P_HI = np.float32(1e-7), np.float32(1.0) - np.float32(1e-7)


def check_oob_args(rf, X) -> np.ndarray:
    if rf.feat is None:
        raise ValueError("the forest is not fitted")
    if not rf.bootstrap:
        raise ValueError("bootstrap=False: every row is in every tree's bag, there is no out-of-bag set")
    X = np.ascontiguousarray(np.asarray(X, dtype=np.uint64).reshape(len(X), -1))
    if rf.n_train is not None and len(X) != rf.n_train:
        raise ValueError(f"out-of-bag evaluation needs the {rf.n_train} training rows, got {len(X)}")
    return X


def oob_predict_proba_numpy(rf, X) -> tuple[np.ndarray, np.ndarray]:
    """(proba [N, 62] float32, count [N] int32) of forest ``rf`` on its training matrix ``X``."""
    from .forest import poisson_weights, unpack_bits

    X = check_oob_args(rf, X)
    n = len(X)
    bits = unpack_bits(X, rf.F)
    acc = np.zeros((n, 64), dtype=np.float32)
    count = np.zeros(n, dtype=np.int32)
    for t in range(len(rf.feat)):
        rows = np.flatnonzero(poisson_weights(rf.seed, rf.tree_start + t, n) == 0)
        node = np.zeros(len(rows), dtype=np.int64)
        for _ in range(rf.max_depth + 1):
            f = rf.feat[t][node]
            act = f >= 0
            if not act.any():
                break
            node[act] = 2 * node[act] + 1 + bits[rows[act], f[act]]
        acc[rows] += rf.value[t][node].astype(np.float32)  # fp32 adds, one tree after the other
        count[rows] += 1
    proba = np.zeros((n, 62), dtype=np.float32)
    has = count > 0
    proba[has] = acc[has, :62] / count[has, None].astype(np.float32)
    return proba, count


def _stable_topk(z: np.ndarray, k: int) -> np.ndarray:
    idx = np.argsort(-z, axis=1, kind="stable")[:, :k]
    m = np.zeros(z.shape, dtype=bool)
    np.put_along_axis(m, idx, True, axis=1)
    return m


def mask_to_bits(Y, n_out: int = 62) -> np.ndarray:
    Y = np.asarray(Y, dtype=np.uint64).reshape(-1)
    return ((Y[:, None] >> np.arange(n_out, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def oob_totals_numpy(proba: np.ndarray, count: np.ndarray, Y) -> dict:
    """The score's totals over the rows with count > 0 (``TOTAL_KEYS`` + ``n``): integers, and the fp64 sums of
    the per-row fp32 Brier and log-loss values."""
    p = np.asarray(proba, dtype=np.float32)[:, :62]
    count = np.asarray(count).reshape(-1)
    y = mask_to_bits(Y)
    use = count > 0
    p, y, c = p[use], y[use], count[use]
    rows = int(use.sum())
    pick = np.concatenate([_stable_topk(p[:, :50], 5), _stable_topk(p[:, 50:], 2)], axis=1) if rows else y
    mism = (pick ^ y).sum(1)
    yf = y.astype(np.float32)
    brier = np.zeros(rows, dtype=np.float32)
    logl = np.zeros(rows, dtype=np.float32)
    pc = np.clip(p, P_LO, P_HI)
    q = np.where(y, pc, np.float32(1.0) - pc).astype(np.float32)
    term = -np.log(q)  # float32
    for j in range(62):  # fp32, ascending j
        d = p[:, j] - yf[:, j]
        brier += d * d
        logl += term[:, j]
    logl = logl / np.float32(62.0)
    return {"rows": rows, "hits_main": int((pick[:, :50] & y[:, :50]).sum()),
            "hits_star": int((pick[:, 50:] & y[:, 50:]).sum()), "exact": int((mism == 0).sum()),
            "mismatch_bits": int(mism.sum()), "target_bits": int(y.sum()), "min_trees": int(c.min()) if rows else 0,
            "trees_sum": int(c.astype(np.int64).sum()), "brier_sum": float(brier.astype(np.float64).sum()),
            "logloss_sum": float(logl.astype(np.float64).sum()), "n": int(len(count))}


def oob_finish(tot: dict) -> dict:
    """Totals -> the out-of-bag score (shared by the numpy and the HIP path)."""
    rows = tot["rows"]
    d = float(rows) if rows else float("nan")
    return {"rows": rows, "rows_without_oob_tree": tot["n"] - rows, "min_trees": tot["min_trees"],
            "mean_trees": tot["trees_sum"] / d, "hits_main": tot["hits_main"] / d, "hits_star": tot["hits_star"] / d,
            "exact": tot["exact"] / d, "acc": (62 * rows - tot["mismatch_bits"]) / (62 * d),
            "trivial_acc": (62 * rows - tot["target_bits"]) / (62 * d), "brier": tot["brier_sum"] / d,
            "logloss": tot["logloss_sum"] / d}


def feature_importances(rf, kind: str = "gain") -> np.ndarray:
    """[F] float64 shares: per feature the sum over the split nodes (feat >= 0) of their gain, of their cover
    (weighted rows) or of 1, normalised to sum 1; all zero if the forest has no split."""
    if rf.feat is None:
        raise ValueError("the forest is not fitted")
    if kind not in ("gain", "cover", "splits"):
        raise ValueError(f"kind must be gain | cover | splits, got {kind!r}")
    split = rf.feat >= 0
    w = {"gain": rf.gain, "cover": rf.cover, "splits": np.ones(rf.feat.shape)}[kind]
    imp = np.bincount(rf.feat[split].astype(np.int64), weights=np.asarray(w, dtype=np.float64)[split], minlength=rf.F)
    imp = imp[:rf.F].astype(np.float64)
    s = imp.sum()
    return imp / s if s > 0 else np.zeros(rf.F, dtype=np.float64)
