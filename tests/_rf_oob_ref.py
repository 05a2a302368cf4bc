"""fp64 reference and comparison rules for the forest's out-of-bag (OOB) evaluation
(tests/test_rf_oob_cpu.py, tests/test_rf_oob_gpu.py).  Nothing in this module touches the GPU.

The reference is written from the definition, one (row, tree) at a time: row i is out of bag for tree t when
``poisson_weights(seed, tree_start + t, N)[i] == 0``; its probability vector is the fp64 mean of the leaf
vectors that a single-row walk reaches in those trees.

Rules:

* counts: equal as integers;
* probabilities: within ``(count + 2) * 2^-24`` per element -- an fp32 implementation does ``count - 1`` adds
  of partial sums <= count and one division, of values in [0, 1]: after the division that is at most
  ``count * 2^-24``;
* rows without an out-of-bag tree: all zero;
* Brier / log-loss sums: within ``k * 2^-24 * sum |term|`` of the fp64 sums over the same fp32 probabilities
  (``metrics_reference``), k = the fp32 operations a term goes through (``K_BRIER``, ``K_LOGLOSS``).
"""
from __future__ import annotations

import numpy as np

from euromillioner_amd.models.forest import poisson_weights

U24 = 2.0 ** -24
# fp32 operations a Brier term (p - y)^2 goes through: the subtraction (its error enters the square twice: 2),
# the multiplication (1) and the at most 61 additions of the row's 62-term sum it takes part in
K_BRIER = 2 + 1 + 61
# ... and a log-loss term -log(q): logf (an error of up to 1 ulp = 2 half-ulps: 2), at most 61 additions, and
# the row's division by 62 (1).  The clamp is exact and the complement q = 1 - p is part of the definition
# (formed in fp32, see models/forest_oob.py), so neither is charged.
K_LOGLOSS = 2 + 61 + 1


# name -> (rows, trees, depth, lags, feature subset, first global tree id or None): rows of the 3000 synthetic
# draws (seed 2, planted 0.7), forest seed 11, fitted by the numpy engine
CASES = {
    "d5": (3000, 10, 5, 1, "sqrt", None),        # streamed form on the device; 38 rows without an OOB tree
    "d6_lags2": (3000, 10, 6, 2, "0.3", None),   # two feature words: the general form
    "t100_d4": (2000, 100, 4, 1, "sqrt", None),  # more than 64 trees
    "t3_d8": (700, 3, 8, 1, "sqrt", None),       # 185 rows without an OOB tree
    "d0": (3000, 10, 0, 1, "sqrt", None),
    "d9": (3000, 10, 9, 1, "sqrt", None),        # one word, too deep for the streamed form
    "range7_12": (1000, 5, 4, 1, "sqrt", 7),     # fit(trees=range(7, 12)): global tree ids
    "n1": (1, 10, 5, 1, "sqrt", None),           # wave and row-group edges
    "n65": (65, 10, 5, 1, "sqrt", None),
    "n1537": (12 * 128 + 1, 10, 5, 1, "sqrt", None),
}
_cache: dict = {}


def build_case(name: str):
    """(forest, X, Y, reference proba, reference count) of CASES[name]; built once per process, read-only."""
    if name not in _cache:
        from euromillioner_amd.data.draws import DrawSet
        from euromillioner_amd.models.forest import RandomForest, draw_features

        n, T, depth, lags, subset, start = CASES[name]
        if ("data", lags) not in _cache:
            _cache["data", lags] = draw_features(DrawSet.synthetic(n=3000, seed=2, planted=0.7, calendar=False).numbers, lags)
        X, Y, F = _cache["data", lags]
        X, Y = X[:n], Y[:n]
        rf = RandomForest(n_trees=T, max_depth=depth, feature_subset=subset, seed=11, device="cpu")
        rf.fit(X, Y, F, trees=None if start is None else range(start, start + T))
        rp, rc = oob_reference(rf.feat, rf.value, depth, rf.seed, start or 0, X)
        for a in (rp, rc):
            a.setflags(write=False)
        _cache[name] = (rf, X, Y, rp, rc)
    return _cache[name]


def walk_row(feat_t, xrow, max_depth: int) -> int:
    """Leaf node of one row (its feature words as Python ints) in one complete-array tree."""
    node = 0
    for _ in range(max_depth + 1):
        f = int(feat_t[node])
        if f < 0:
            break
        node = 2 * node + 1 + ((xrow[f >> 6] >> (f & 63)) & 1)
    return node


def oob_reference(feat, value, max_depth: int, seed: int, tree_start: int, X) -> tuple[np.ndarray, np.ndarray]:
    """(proba [N, 62] float64, count [N] int64) from the definition."""
    X = np.asarray(X, dtype=np.uint64).reshape(len(X), -1)
    n, T = len(X), len(feat)
    w = [poisson_weights(seed, tree_start + t, n) for t in range(T)]
    rows = [[int(v) for v in r] for r in X]
    proba = np.zeros((n, 62), dtype=np.float64)
    count = np.zeros(n, dtype=np.int64)
    for i in range(n):
        s = np.zeros(62, dtype=np.float64)
        c = 0
        for t in range(T):
            if w[t][i] != 0:
                continue
            s += value[t][walk_row(feat[t], rows[i], max_depth)][:62].astype(np.float64)
            c += 1
        count[i] = c
        if c:
            proba[i] = s / c
    return proba, count


def check_oob(proba, count, ref_proba, ref_count) -> float:
    """The rules above for an implementation's (proba [N, >= 62], count [N]); returns the worst error / budget."""
    proba = np.asarray(proba)
    count = np.asarray(count)
    assert proba.shape[0] == len(ref_count) and count.shape == ref_count.shape, (proba.shape, count.shape)
    assert np.issubdtype(count.dtype, np.integer), count.dtype
    assert np.array_equal(count.astype(np.int64), ref_count), {"rows_with_wrong_count": int((count != ref_count).sum())}
    assert not np.isnan(proba).any()
    zero = ref_count == 0
    assert not proba[zero].any(), "rows without an out-of-bag tree must be all zero"
    if proba.shape[1] > 62:
        assert not proba[:, 62:].any(), "outputs 62 and 63 must be zero"
    err = np.abs(proba[:, :62].astype(np.float64) - ref_proba)
    budget = (ref_count + 2)[:, None] * U24
    worst = float((err / budget).max()) if err.size else 0.0
    assert worst <= 1.0, {"worst_error_over_budget": worst, "max_err": float(err.max())}
    return worst


def metrics_reference(proba32, count, Y) -> dict:
    """Totals of the OOB score over the rows with count > 0, from the definition, on fp32 probabilities:
    integers exactly; ``brier_sum`` / ``logloss_sum`` in fp64 with their budgets ``*_budget``
    (``k * 2^-24 * sum |term|``; a log-loss term is its share 1/62 of the row's value)."""
    p32 = np.asarray(proba32, dtype=np.float32)[:, :62]
    count = np.asarray(count).reshape(-1)
    Y = np.asarray(Y, dtype=np.uint64).reshape(-1)
    tot = {"rows": 0, "hits_main": 0, "hits_star": 0, "exact": 0, "mismatch_bits": 0, "target_bits": 0,
           "min_trees": 0, "trees_sum": 0, "n": int(len(count))}
    brier = logl = brier_abs = logl_abs = 0.0
    lo, hi = np.float32(1e-7), np.float32(1.0) - np.float32(1e-7)
    cmin = None
    for i in range(len(count)):
        c = int(count[i])
        if c <= 0:
            continue
        p = p32[i]
        yi = int(Y[i])
        y = [(yi >> j) & 1 for j in range(62)]
        pl = [float(v) for v in p]
        pick = sorted(range(50), key=lambda j: (-pl[j], j))[:5] + sorted(range(50, 62), key=lambda j: (-pl[j], j))[:2]
        pm = [0] * 62
        for j in pick:
            pm[j] = 1
        mism = sum(a != b for a, b in zip(pm, y))
        tot["rows"] += 1
        tot["hits_main"] += sum(pm[j] & y[j] for j in range(50))
        tot["hits_star"] += sum(pm[j] & y[j] for j in range(50, 62))
        tot["exact"] += int(mism == 0)
        tot["mismatch_bits"] += mism
        tot["target_bits"] += sum(y)
        tot["trees_sum"] += c
        cmin = c if cmin is None else min(cmin, c)
        ya = np.array(y, dtype=np.float64)
        bt = (p.astype(np.float64) - ya) ** 2
        pc = np.clip(p, lo, hi)  # fp32, exact
        q = np.where(ya > 0, pc, np.float32(1.0) - pc).astype(np.float32)  # the complement: fp32 by definition
        lt = -np.log(q.astype(np.float64)) / 62.0
        brier += float(bt.sum())
        logl += float(lt.sum())
        brier_abs += float(np.abs(bt).sum())
        logl_abs += float(np.abs(lt).sum())
    tot["min_trees"] = cmin or 0
    tot.update(brier_sum=brier, logloss_sum=logl, brier_budget=K_BRIER * U24 * brier_abs,
               logloss_budget=K_LOGLOSS * U24 * logl_abs)
    return tot


INT_KEYS = ("rows", "hits_main", "hits_star", "exact", "mismatch_bits", "target_bits", "min_trees", "trees_sum", "n")


def check_totals(got: dict, ref: dict) -> None:
    """An implementation's totals against ``metrics_reference`` of ITS OWN fp32 probabilities."""
    for k in INT_KEYS:
        assert int(got[k]) == int(ref[k]), (k, got[k], ref[k])
    for k in ("brier", "logloss"):
        err = abs(float(got[k + "_sum"]) - ref[k + "_sum"])
        print(f"{k}_sum: err {err:.3e} budget {ref[k + '_budget']:.3e}")
        assert err <= ref[k + "_budget"], (k, err, ref[k + "_budget"])


def finish_reference(ref: dict) -> dict:
    """The score dict of ``metrics_reference``'s totals, with ``brier_budget`` / ``logloss_budget`` per row."""
    rows = ref["rows"]
    return {"rows": rows, "rows_without_oob_tree": ref["n"] - rows, "min_trees": ref["min_trees"],
            "mean_trees": ref["trees_sum"] / rows, "hits_main": ref["hits_main"] / rows,
            "hits_star": ref["hits_star"] / rows, "exact": ref["exact"] / rows,
            "acc": (62 * rows - ref["mismatch_bits"]) / (62 * rows),
            "trivial_acc": (62 * rows - ref["target_bits"]) / (62 * rows), "brier": ref["brier_sum"] / rows,
            "logloss": ref["logloss_sum"] / rows, "brier_budget": ref["brier_budget"] / rows,
            "logloss_budget": ref["logloss_budget"] / rows}


SCORE_KEYS = ("rows", "rows_without_oob_tree", "min_trees", "mean_trees", "hits_main", "hits_star", "exact", "acc",
              "trivial_acc", "brier", "logloss")


def check_score(got: dict, ref_score: dict) -> None:
    """A score dict against ``finish_reference``: the integer-derived keys to 1e-12, the two sums to their budgets."""
    assert set(got) == set(SCORE_KEYS), sorted(got)
    for k in SCORE_KEYS:
        tol = ref_score[k + "_budget"] if k in ("brier", "logloss") else 1e-12
        assert abs(float(got[k]) - float(ref_score[k])) <= tol, (k, got[k], ref_score[k], tol)
