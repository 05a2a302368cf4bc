"""The fits of tests/test_gbdt_fit_gpu.py, shared with tests/test_gbdt_fit_ref_cpu.py, which runs the reference
on the numpy engine's trees of the same cases: the ambiguity cap of the GPU tests is a condition on the inputs,
and the inputs are chosen so that the reference alone stays inside it.

A case is (data name, objective, keyword arguments of ``GBDT``); ``data(name)`` returns (X, Y, ties), ``ties``
being the pairs of columns with identical bins.  Chunk counts of the row-count cases come from ``plan_hist`` in
``csrc/gbdt.hip``: ``chunk = max(HIST_MIN_CHUNK, ceil(n / ceil(4096 / T)))`` rows, ``ceil(n / chunk)`` chunks:

    n = 8, 255, 256 (T = 5)  1 chunk    no fold
    n = 257 (T = 5)          2 chunks   partials staged at once
    n = 6400 (T = 5)         25 chunks  per-cell chunk loop (25 x 124 cells x 16 B > SPLIT_ONESHOT_LDS)
    n = 8448 (T = 2)         33 chunks  gbdt_chunk_reduce (> SPLIT_FOLD_MAX_CHUNKS)
"""
from __future__ import annotations

import functools

import numpy as np

import _gbdt_watch_data as D

STD = dict(D.KW)  # nround 12, depth 3, eta 0.5, gamma 0
HIST_MIN_CHUNK, BLOCKS_PER_LEVEL = 256, 4096
ROWS_SEED = 37  # (a seed at which no side of the 255 to 257-row fits has an H within rounding of min_child_weight)
ROWS = {8: (5, 1), 255: (5, 1), 256: (5, 1), 257: (5, 2), 6400: (5, 25), 8448: (2, 33)}  # n -> (T, chunks)


def chunks_of(n: int, T: int) -> int:
    per_task = -(-BLOCKS_PER_LEVEL // T)
    chunk = max(HIST_MIN_CHUNK, -(-n // per_task))
    return -(-n // chunk)


def _classes(X):
    """Four classes from three columns (the rule of test_gbdt._multi_data)."""
    y = (X[:, 0] > 0).astype(np.int64) + 2 * (X[:, 1] > 0.4) + (X[:, 2] > 1.2)
    return np.minimum(y, 3).astype(np.float64)


@functools.lru_cache(maxsize=None)
def data(name: str):
    """(X, Y, ties).  Names: std / std2 (2 tasks) / multi (the standard problems), rows<n>, t62, mixed (5a),
    mixed-multi, cont (5b), cont-multi, cont650 (the lambda = 0 case), int8 (5c), edge (5d)."""
    if name == "std":
        return (*D.problem("reg:logistic")["train"], ())
    if name == "std2":
        X, Y = D.problem("reg:logistic")["train"]
        return X, Y[:, [1, 3]].copy(), ()  # (task 0 has a 4-row side whose H sits on min_child_weight)
    if name == "multi":
        return (*D.problem("multi:softprob")["train"], ())
    if name.startswith("rows"):
        n = int(name[4:])
        X, Y, _ = D._draws(n, ROWS_SEED, ROWS[n][0])
        return X, Y, ()
    if name == "t62":
        return (*D.large_problem()["small"], ())
    if name in ("mixed", "mixed-multi"):
        # the reference feature set: 63 two-valued columns + month, day, year (12, 31, 13 bins on these rows)
        from euromillioner_amd import config as C
        from euromillioner_amd.data.draws import DrawSet
        from euromillioner_amd.pipeline import gbdt_dataset

        X, Y, _ = gbdt_dataset(DrawSet.synthetic(n=901, seed=8, planted=0.6, calendar=True), C.RunConfig())
        X, Y = np.asarray(X, np.float64)[:900], np.asarray(Y, np.float64)[:900]
        if name == "mixed":
            return X, Y[:, :5].copy(), ()
        return X, Y[:, 0] + 2 * Y[:, 1], ()
    if name in ("cont", "cont-multi", "cont650"):  # 12 continuous features, 256 bins each
        # (seeds at which the numpy engine's trees have no near-tie: tiny depth-6 nodes tie easily)
        rng = np.random.default_rng(7 if name == "cont650" else 1)
        n = 650 if name == "cont650" else 1500
        X = rng.normal(size=(n, 12))
        if name == "cont-multi":
            return X, _classes(X), ()
        y = ((X[:, 0] + 0.5 * X[:, 3] * X[:, 5] + 0.3 * rng.normal(size=n)) > 0).astype(np.float64)
        y2 = ((X[:, 1] - X[:, 2] + 0.5 * rng.normal(size=n)) > 0.3).astype(np.float64)
        return X, np.stack([y, y2], axis=1), ()
    if name == "int8":  # 6 integer features of 8 values: every feature within SPLIT_DIRECT_MAX_BINS
        rng = np.random.default_rng(5)
        X = rng.integers(0, 8, size=(257, 6)).astype(np.float64)
        z = X[:, 0] - X[:, 1] + 0.5 * X[:, 2] + rng.normal(size=257)
        Y = np.stack([(z > 0), (X[:, 3] + X[:, 4] > 7), (z + X[:, 5] > 4)], axis=1).astype(np.float64)
        return X, Y, ()
    if name == "edge":
        # the standard problem with a constant column first and last, a two-valued column and a copy of a
        # one-hot column: columns [const, 62 one-hot, two-valued, copy of a one-hot column, const]
        X, Y = D.problem("reg:logistic")["train"]
        n = len(X)
        two = np.where(X[:, 3] + X[:, 17] + X[:, 40] > 0, 7.0, -3.0)
        dup = _most_telling_column(X, Y)
        Xe = np.concatenate([np.full((n, 1), 2.5), X, two[:, None], X[:, dup:dup + 1], np.full((n, 1), -1.0)], axis=1)
        return Xe, Y, ((1 + dup, 64),)
    raise KeyError(name)


def _most_telling_column(X, Y) -> int:
    """The column with the largest |correlation| to one of the labels: the trees split on it, so its copy ties."""
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    c = np.abs(Xc.T @ Yc) / (np.sqrt((Xc ** 2).sum(0))[:, None] * np.sqrt((Yc ** 2).sum(0))[None, :] + 1e-30)
    return int(np.argmax(c.max(axis=1)))


EDGE_CONST = (0, 65)

P_ZERO = dict(reg_lambda=0.0, min_child_weight=0.0, gamma=0.0, eta=0.5, base_score=0.5, nround=3)
P_HEAVY = dict(reg_lambda=3.5, min_child_weight=5.0, gamma=0.0, eta=0.3, base_score=0.2)
P_REF = dict(reg_lambda=1.0, min_child_weight=1.0, gamma=1.0, eta=1.0, base_score=0.5)
ROW_KW = dict(nround=3)
LOG, SQ, SOFT = "reg:logistic", "reg:squarederror", "multi:softprob"


def kw_of(**kw):
    return dict(STD, **kw)


# name -> (data, objective, kwargs); the drivers, the process group and the chunked calls are the GPU test's
CASES = {
    "std-logistic": ("std", LOG, kw_of()),
    "std-squarederror": ("std", SQ, kw_of()),
    "std-softprob": ("multi", SOFT, kw_of()),
    "par-zero": ("cont650", LOG, kw_of(**P_ZERO)),
    "par-heavy": ("std", LOG, kw_of(**P_HEAVY)),
    "par-ref": ("std", LOG, kw_of(**P_REF)),
    **{f"depth-{d}": ("std2", LOG, kw_of(max_depth=d, nround=2)) for d in (1, 6, 8, 9)},
    **{f"rows-{n}": (f"rows{n}", LOG, kw_of(**ROW_KW)) for n in ROWS},
    "mixed": ("mixed", LOG, kw_of()),
    "cont": ("cont", LOG, kw_of(max_depth=6, nround=4)),
    "int8": ("int8", LOG, kw_of()),
    "edge": ("edge", LOG, kw_of()),
    "quant-std-logistic": ("std", LOG, kw_of(hist_mode="quant")),
    "quant-std-softprob": ("multi", SOFT, kw_of(hist_mode="quant")),
    "quant-mixed-logistic": ("mixed", LOG, kw_of(hist_mode="quant")),
    "quant-mixed-softprob": ("mixed-multi", SOFT, kw_of(hist_mode="quant")),
    "quant-cont-logistic": ("cont", LOG, kw_of(hist_mode="quant", max_depth=6, nround=4)),
    "quant-cont-softprob": ("cont-multi", SOFT, kw_of(hist_mode="quant", max_depth=6, nround=4)),
    "sub-0.5-logistic": ("std", LOG, kw_of(subsample=0.5, seed=0)),
    "sub-0.8-logistic": ("std", LOG, kw_of(subsample=0.8, seed=12345)),
    "sub-0.5-squarederror": ("std", SQ, kw_of(subsample=0.5, seed=12345)),
    "sub-0.8-quant": ("std", LOG, kw_of(subsample=0.8, seed=12345, hist_mode="quant")),
    "sub-0.5-quant": ("std", LOG, kw_of(subsample=0.5, seed=0, hist_mode="quant")),
    "sub-0.5-softprob": ("multi", SOFT, kw_of(subsample=0.5, seed=0)),
    "sub-0.8-softprob": ("multi", SOFT, kw_of(subsample=0.8, seed=12345)),
    "sub-0.8-rounds7": ("std", LOG, kw_of(subsample=0.8, seed=12345, nround=7)),
    "sub-0.5-rounds7": ("std", LOG, kw_of(subsample=0.5, seed=0, nround=7)),
    "t62": ("t62", LOG, kw_of(nround=3)),
    # no element survives u < float32(1e-9) (u is a multiple of 2^-24): every tree's root has H + lambda = 0
    "dropped-all": ("rows8", LOG, kw_of(subsample=1e-9, reg_lambda=0.0, min_child_weight=0.0, nround=2)),
}


def partial_gamma(gains) -> float:
    """The median split gain of a gamma = 0 fit, moved half-way to the next larger gain so that no split sits
    on the threshold itself."""
    g = np.unique(np.asarray(gains, np.float64))
    i = (len(g) - 1) // 2
    return float(0.5 * (g[i] + g[i + 1]))


def cap(res) -> int:
    return max(1, res.decisions // 100)
