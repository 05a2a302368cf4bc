"""Training sets and the small fit cases shared by ``test_rf_fit_ref_cpu.py`` (``check_forest`` accepts the numpy
engine on them) and ``test_rf_fit_gpu.py`` (the device driver on the same cases, and on the larger ones there)."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from euromillioner_amd.data.draws import DrawSet
from euromillioner_amd.models.forest import draw_features, n_candidates


@lru_cache(maxsize=None)
def draws_data(n: int, lags: int = 1):
    """Exactly n rows of the planted synthetic draws (one-hot features split about 90 / 10: one node of every
    level stays large)."""
    ds = DrawSet.synthetic(n=n + lags + 1, seed=2, planted=0.7, calendar=False)
    X, Y, F = draw_features(ds.numbers, lags)
    X, Y = np.ascontiguousarray(X[:n]), np.ascontiguousarray(Y[:n])
    assert len(X) == n and len(Y) == n
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, F


@lru_cache(maxsize=None)
def mask_form_data(n: int, ymax: int):
    """The generator of ``test_forest.py::test_hip_forest_record_forms_match_oracle``: rows with up to ymax - 1
    outputs (more than 7 somewhere: mask-form records), balanced feature bits."""
    rng = np.random.default_rng(ymax)
    X = np.zeros(n, dtype=np.uint64)
    Y = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        for b in rng.choice(62, size=int(rng.integers(0, 12)), replace=False):
            X[i] |= np.uint64(1) << np.uint64(b)
        for b in rng.choice(62, size=int(rng.integers(0, ymax)), replace=False):
            Y[i] |= np.uint64(1) << np.uint64(b)
        if i % 3 == 0:  # a learnable output
            Y[i] |= (X[i] & np.uint64(1)) << np.uint64(5)
    X = X.reshape(-1, 1)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, 62


@lru_cache(maxsize=None)
def dense_data(n: int, F: int):
    """Random dense bits, F of them in ONE word (62: record form; 63, 64: bits 62 / 63 are features, not the
    weight).  Outputs 0, 1, 2 equal feature bits 61, 62, 63 (those below F); outputs 3..9 are noise."""
    assert 62 <= F <= 64
    rng = np.random.default_rng(F)
    bits = rng.integers(0, 2, size=(n, 64)).astype(np.uint64)
    bits[:, F:] = 0
    X = (bits << np.arange(64, dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)
    Y = np.zeros(n, dtype=np.uint64)
    for o, f in enumerate((61, 62, 63)):
        if f < F:
            Y |= bits[:, f] << np.uint64(o)
    Y |= (rng.integers(0, 2 ** 7, size=n).astype(np.uint64) & rng.integers(0, 2 ** 7, size=n).astype(np.uint64)) << np.uint64(3)
    X = X.reshape(-1, 1)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, F


def degenerate_data(kind: str):
    X, Y, F = draws_data(64, 1)
    if kind == "identical":
        return np.repeat(X[:1], 64, axis=0), np.repeat(Y[:1], 64), F
    if kind == "y_zero":
        return X, np.zeros_like(Y), F
    if kind == "x_zero":
        return np.zeros_like(X), Y, F
    raise ValueError(kind)


class Case:
    """One fit: data = (kind, *args) for :func:`data_of`; trees = (first global id, count)."""

    def __init__(self, name, data, depth, trees, subset, bootstrap, min_leaf=1, seed=11):
        self.name, self.data, self.depth, self.subset = name, data, depth, subset
        self.trees = range(trees[0], trees[0] + trees[1])
        self.bootstrap, self.min_leaf, self.seed = bootstrap, min_leaf, seed

    def load(self):
        X, Y, F = data_of(self.data)
        return X, Y, F, n_candidates(self.subset, F)

    def __repr__(self):
        return self.name


def data_of(spec):
    kind, *a = spec
    if kind == "draws":
        return draws_data(*a)
    if kind == "mask":
        return mask_form_data(*a)
    if kind == "dense":
        return dense_data(*a)
    if kind == "tiny":
        X, Y, F = draws_data(64, 1)
        return X[:a[0]], Y[:a[0]], F
    return degenerate_data(kind)


def _small_cases():
    c = []
    for ml in (5, 25, 400):
        for boot in (True, False):
            c.append(Case(f"minleaf{ml}-{'boot' if boot else 'all'}", ("draws", 3000, 1), 6, (0, 4), "sqrt", boot, ml))
    c.append(Case("ids5to10", ("draws", 3000, 1), 5, (5, 6), "sqrt", True))
    c.append(Case("shard0to3", ("draws", 3000, 1), 5, (0, 3), "sqrt", True))
    c.append(Case("shard3to6", ("draws", 3000, 1), 5, (3, 3), "sqrt", True))
    for F in (62, 63, 64):
        c.append(Case(f"dense{F}", ("dense", 3000, F), 5, (0, 4), "all", False))
    c.append(Case("lags2-index", ("draws", 2000, 2), 5, (0, 4), "0.3", True, 3))
    c.append(Case("lags3", ("draws", 3000, 3), 5, (0, 4), "0.3", True))
    c.append(Case("lags4-all", ("draws", 3000, 4), 5, (0, 4), "all", False))
    for boot in (True, False):
        b = "boot" if boot else "all"
        for n in (1, 2, 3, 4):
            c.append(Case(f"n{n}-{b}", ("tiny", n), 3, (0, 4), "sqrt", boot))
        for kind in ("identical", "y_zero", "x_zero"):
            c.append(Case(f"{kind}-{b}", (kind,), 3, (0, 4), "sqrt", boot))
    return c


SMALL_CASES = _small_cases()
