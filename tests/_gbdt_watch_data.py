"""The problems and watch lists shared by tests/test_gbdt_ref_cpu.py and tests/test_gbdt_watch_gpu.py.

The standard watch list is ``train`` (the training rows), ``one`` (1 row), ``a`` (255 rows), ``b`` (257 rows:
one block of 256 elements per task plus one), then ``big`` (more rows than the training set, so it fixes the
stride of the per-set metric partials) and ``c``.  Four sets keep the engine's deferred metrics, five and six
leave them.

Each set ends in its hardest row, one no model of these data predicts: a metric that loses its tail shows in
the error counts only if the tail holds an error."""
from __future__ import annotations

import numpy as np

N_TRAIN = 650
SIZES = {"one": 1, "a": 255, "b": 257, "big": 700, "c": 103}
ORDER = ("train", "one", "a", "b", "big", "c")
KW = dict(nround=12, max_depth=3, eta=0.5, gamma=0.0)
# (objective, eval_metric) pairs of the matrix; the multi-class rows have one class id per row
PAIRS = (("reg:logistic", "logloss"), ("reg:logistic", "error"), ("reg:squarederror", "rmse"),
         ("reg:squarederror", "error"), ("multi:softprob", "mlogloss"), ("multi:softprob", "merror"))
N_LARGE = 17000  # 62 tasks x 17 000 rows = 1 054 000 elements > 4096 blocks x 256 threads
N_LARGE_TRAIN = 600


def _split(X, Y, sizes, score):
    """Consecutive row ranges; each set's row of the largest ``score`` is swapped to its end."""
    out, o = {}, 0
    for name, k in sizes:
        xs, ys = X[o:o + k].copy(), Y[o:o + k].copy()
        j = int(np.argmax(score[o:o + k]))
        xs[[j, k - 1]], ys[[j, k - 1]] = xs[[k - 1, j]], ys[[k - 1, j]]
        out[name] = (xs, ys)
        o += k
    assert o <= len(X)
    return out


def _draws(total: int, seed: int, T: int):
    """Next-draw multi-hot problem (as tests/test_trees_property_gpu.py) and the rows' hardness: the number of
    positive labels the planted permutation does not explain (the last task's counted 100-fold, so the very
    last element of a set is such a label wherever the set has one)."""
    from euromillioner_amd.data.draws import DrawSet, multi_hot

    ds = DrawSet.synthetic(n=total + 1, seed=seed, planted=0.8, calendar=False)
    X = multi_hot(ds.numbers[:-1]).astype(np.float64)
    Y = multi_hot(ds.numbers[1:]).astype(np.float64)
    perm = np.asarray(ds.meta["perm"], dtype=np.int64)  # number j + 1 -> perm[j] (mains), star j + 1 -> perm[50 + j]
    pred = np.zeros_like(Y)
    pred[:, perm[:50] - 1] = X[:, :50]
    pred[:, 50 + perm[50:] - 1] = X[:, 50:]
    noise = ((Y == 1) & (pred == 0))[:, :T].astype(np.float64)
    return X, Y[:, :T], 100.0 * noise[:, -1] + noise.sum(axis=1)


def problem(objective: str, seed: int = 11, T: int = 5):
    """{"train": (X, Y), "one": ..., ...}: every set of ORDER, disjoint rows of one synthetic data set."""
    sizes = [("train", N_TRAIN)] + [(k, SIZES[k]) for k in ORDER[1:]]
    total = sum(k for _, k in sizes)
    if objective.startswith("multi:"):
        from test_gbdt import _multi_data

        X, Y = _multi_data(total, seed=seed)
        # the row just below _multi_data's sparsest class boundary (x2 > 1.2: the trees cut a little below it)
        d = 1.2 - X[:, 2]
        return _split(X, Y, sizes, np.where(d > 0, -d, -np.inf))
    X, Y, score = _draws(total, seed, T)
    return _split(X, Y, sizes, score)


def watch(sets: dict, n_sets: int) -> dict:
    """The first ``n_sets`` sets of ORDER as an evals dict (``train`` first)."""
    return {k: sets[k] for k in ORDER[:n_sets]}


def large_problem(seed: int = 12):
    """62 tasks: ``small`` (600 rows), ``large`` (17 000 rows) and ``b`` (257 rows)."""
    sizes = [("small", N_LARGE_TRAIN), ("large", N_LARGE), ("b", 257)]
    X, Y, score = _draws(sum(k for _, k in sizes), seed, 62)
    return _split(X, Y, sizes, score)


def refs_for(R, model, evals: dict, train=None) -> dict:
    """The reference of every watch set (and, with ``train = (X, Y)``, of the train metric under R.TRAIN) from
    the model's own trees and cuts."""
    out = {}
    pairs = list(evals.items()) + ([(R.TRAIN, train)] if train is not None else [])
    for name, (ex, ey) in pairs:
        m = R.margins_by_round(model.trees, model.cuts, model.n_tasks, model.base_margin, ex)
        out[name] = R.reference(model.objective, model.eval_metric, ey, m)
    return out
