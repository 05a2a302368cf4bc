"""The yardstick of the forest contributions (``RandomForest.predict_contribs``): fp64 Shapley values from the
definition, and the error budget of a float32 engine.

Numpy only, and independent of ``euromillioner_amd/models/forest_explain.py``.

The game.  Features are binary; a split node ``i`` on ``f`` sends bit 0 to ``2i+1`` and bit 1 to ``2i+2``; a node
with ``feat < 0`` is a leaf with a 62-vector.  For a set ``S`` of known features, a split on a feature in ``S``
follows the row, any other split averages its children with ``cover[child] / cover[node]``: the stored float32
covers (the values a device engine holds), divided in fp64.  ``predict_proba`` is the mean over the ``T`` trees, so
every tree's values are divided by ``T``; the bias column is ``v({})``.

Two references:

* :func:`shapley_trees` (a): per tree, all subsets of the features the tree uses, through
  ``_gbdt_shap_ref.shapley`` unchanged, fed the forest recast as 62 x T single-output trees (tree ``t``, output
  ``o`` -> recast tree ``62 t + o`` of task ``o``; status 1 / 2, ``sbin`` 0, bits as bins), divided by ``T``.
  Only for shallow trees: a tree must use few features.
* :func:`shapley_leaves` (b): by linearity of the Shapley value a tree's game is the sum of its leaves' games;
  leaf ``L`` with path features ``f_1 .. f_d`` (distinct) is the game ``v_L(S) = value[L] * prod_{j in S} o_j *
  prod_{j not in S} z_j`` over its own ``d <= 8`` players, enumerated over all ``2^d`` subsets.

Budget.  :func:`budget` is the largest ``|engine - reference|`` allowed per output element, from the reference's own
values only, in the manner of ``_gbdt_shap_ref.budget``: ``u = 2^-24``, ``g(k) = k u / (1 - k u)``.  An engine
evaluates, per (row, leaf, path feature ``i``), ``term = value / T * (o_i - z_i) * sum_s w_s c_s`` in float32 and adds
the ``N`` terms of an output column in float32.  ``A`` is the same sum with every term replaced by its absolute value
(``o_i - z_i -> o_i + z_i``), including the 1/T.  Roundings of one term, each relative to the term's magnitude, with
``D`` = max_depth and distinct path features:

* the ``z_j``: one float32 division per edge, at most ``D`` over the path;
* the coefficients ``c_s``: ``d - 1`` factors, each one product and one (fused multiply-)add per coefficient, all
  operands non-negative: at most ``2 (D - 1)``;
* ``sum_s w_s c_s``: the rounding of ``w_s``, the product, ``d - 1`` additions of non-negative values: ``D + 1``;
* ``(o_i - z_i) * w * value``: 3;
* the 1/T: 1.

That is ``c(D) = 4 D + 3`` per term; the float32 accumulation adds ``N - 1``; storing as float32 is covered by a last
``2^-23 |ref|``:

    budget = g(N + 4 D + 3) * A + 2^-23 * |ref|.

``N`` is counted per column: the leaves whose path crosses the feature (for the bias column, all the leaves).  A
column no path crosses has ``A = 0``, ``ref = 0`` and budget 0: it must be exactly 0.  The constant comes from this
count, not from any engine's error.
"""
from __future__ import annotations

import math
import types

import numpy as np

import _gbdt_shap_ref as S

U32 = 2.0 ** -24
N_OUT = 62


def bits_of(X, F: int) -> np.ndarray:
    """[n, F] int64 bits of packed rows [n, W] uint64."""
    X = np.asarray(X, dtype=np.uint64).reshape(len(X), -1)
    return np.stack([((X[:, f // 64] >> np.uint64(f % 64)) & np.uint64(1)).astype(np.int64) for f in range(F)], axis=1)


def leaf_paths(feat, cover):
    """[(tree, leaf node, [(feature, side, z)])] by descending from each root; z the fp64 quotient of the float32 covers."""
    out = []
    cover = np.asarray(cover, dtype=np.float32)

    def go(t, i, path):
        f = int(feat[t, i])
        if f < 0:
            out.append((t, i, path))
            return
        for side in (0, 1):
            c = 2 * i + 1 + side
            go(t, c, path + [(f, side, float(cover[t, c]) / float(cover[t, i]))])

    for t in range(feat.shape[0]):
        go(t, 0, [])
    return out


# ----------------------------------------------------------------------------- (a) tree-level, by the definition
def recast(rf):
    """The forest as 62 x T single-output heap trees in the GBDT reference's arrays."""
    feat = np.asarray(rf.feat)
    T, NN = feat.shape
    status = np.zeros((T, NN), dtype=np.int8)
    for t, i, path in leaf_paths(feat, rf.cover):
        status[t, i] = 2
        while i > 0:
            i = (i - 1) // 2
            status[t, i] = 1
    tr = types.SimpleNamespace(
        status=np.repeat(status, N_OUT, axis=0), feat=np.repeat(feat.astype(np.int64), N_OUT, axis=0),
        leaf=np.asarray(rf.value, np.float64)[:, :, :N_OUT].transpose(0, 2, 1).reshape(T * N_OUT, NN),
        cover=np.repeat(np.asarray(rf.cover, np.float32).astype(np.float64), N_OUT, axis=0))
    return tr, np.zeros((T * N_OUT, NN), dtype=np.int64)


def shapley_trees(rf, X) -> np.ndarray:
    """fp64 ``[n, 62, F+1]``: reference (a)."""
    tr, sbin = recast(rf)
    return S.shapley(tr, sbin, bits_of(X, rf.F), N_OUT, 0.0) / len(rf.feat)


# ----------------------------------------------------------------------------- (b) the per-leaf game
def _leaf_game(path, bits):
    """(w_plus [d, n], w_abs [d, n], pz): per path feature i the Shapley weight of the unit leaf
    sum_S w(|S|) (v(S + i) - v(S)) over all subsets S of the other features, the same with
    |o_i - z_i| -> o_i + z_i, and prod z."""
    d, n = len(path), bits.shape[0]
    z = np.array([p[2] for p in path])
    o = np.stack([(bits[:, f] == side).astype(np.float64) for f, side, _ in path]) if d else np.zeros((0, n))
    P = np.ones((1, n))  # P[m] = prod_{j in m} o_j * prod_{j not in m} z_j, every subset m of the d players
    for j in range(d):
        P = np.concatenate([P * z[j], P * o[j][None, :]])  # bit j of m clear | set
    masks = np.arange(1 << d)
    size = np.array([bin(int(m)).count("1") for m in masks])
    w = np.array([math.factorial(s) * math.factorial(d - 1 - s) / math.factorial(d) for s in range(d)])
    plus, absw = np.zeros((d, n)), np.zeros((d, n))
    for i in range(d):
        m = masks[((masks >> i) & 1) == 0]
        ws = w[size[m]][:, None]
        plus[i] = (ws * (P[m | (1 << i)] - P[m])).sum(axis=0)
        absw[i] = (ws * (P[m | (1 << i)] + P[m])).sum(axis=0)
    return plus, absw, float(np.prod(z)) if d else 1.0


def shapley_leaves(rf, X, with_budget: bool = True):
    """``(ref, budget)``, both fp64 ``[n, 62, F+1]``: reference (b) and the budget of the module docstring."""
    bits = bits_of(X, rf.F)
    n, F, T = len(bits), rf.F, len(rf.feat)
    ref = np.zeros((n, N_OUT, F + 1))
    A = np.zeros((n, N_OUT, F + 1))
    N = np.zeros(F + 1, dtype=np.int64)
    value = np.asarray(rf.value, dtype=np.float64)
    for t, i, path in leaf_paths(np.asarray(rf.feat), rf.cover):
        v = value[t, i, :N_OUT] / T
        plus, absw, pz = _leaf_game(path, bits)
        ref[:, :, F] += v * pz
        A[:, :, F] += np.abs(v) * pz
        N[F] += 1
        for j, (f, _, _) in enumerate(path):
            ref[:, :, f] += plus[j][:, None] * v[None, :]
            A[:, :, f] += absw[j][:, None] * np.abs(v)[None, :]
            N[f] += 1
    if not with_budget:
        return ref
    return ref, budget(ref, A, N, rf.max_depth)


def budget(ref, A, N, max_depth: int) -> np.ndarray:
    k = (N + 4 * int(max_depth) + 3).astype(np.float64) * U32
    return (k / (1.0 - k))[None, None, :] * A + 2.0 ** -23 * np.abs(ref)


worst_ratio = S.worst_ratio
violations = S.violations


# ----------------------------------------------------------------------------- plain walks
def heap_walk(rf, X) -> np.ndarray:
    """int [n, T]: where each row stops in each tree, one row and one tree at a time."""
    bits = bits_of(X, rf.F)
    out = np.zeros((len(bits), len(rf.feat)), dtype=np.int64)
    for t in range(len(rf.feat)):
        for r in range(len(bits)):
            i = 0
            while rf.feat[t][i] >= 0:
                i = 2 * i + 1 + int(bits[r, rf.feat[t][i]])
            out[r, t] = i
    return out


def proba64(rf, X) -> np.ndarray:
    """fp64 ``[n, 62]`` mean leaf vector over the trees."""
    at = heap_walk(rf, X)
    value = np.asarray(rf.value, dtype=np.float64)
    return np.mean([value[t][at[:, t], :N_OUT] for t in range(len(rf.feat))], axis=0)


# ----------------------------------------------------------------------------- the cases both test files share
# name -> (depth, trees, draws fitted on, lags, rows explained, min_samples_leaf): the 3000 synthetic draws of the
# out-of-bag tests (seed 2, planted 0.7), forest seed 11, fitted by the numpy engine.  The one-word cases also
# explain the all-zero row and the row with all 62 bits set.
CASES = {
    "d3": (3, 4, 400, 1, 130, 1),       # two full 64-row groups plus 2; small enough for reference (a)
    "d8": (8, 6, 3000, 1, 65, 1),       # paths of 8 features, a leaf count that is no multiple of 64
    "d0": (0, 3, 3000, 1, 5, 1),        # bare roots: bias only
    "d1": (1, 1, 3000, 1, 1, 1),
    "minleaf": (8, 5, 1000, 1, 64, 50),  # leaves at every depth from 1 to 8
    "lags2": (6, 5, 3000, 2, 63, 1),    # two feature words
    "lags4": (4, 2, 3000, 4, 3, 1),     # four feature words: the largest accumulator tile
}
_cache: dict = {}


def data(lags: int):
    """(X, Y, F) of the 3000 synthetic draws at ``lags``."""
    if ("data", lags) not in _cache:
        from euromillioner_amd.data.draws import DrawSet
        from euromillioner_amd.models.forest import draw_features

        _cache["data", lags] = draw_features(DrawSet.synthetic(n=3000, seed=2, planted=0.7, calendar=False).numbers, lags)
    return _cache["data", lags]


def build_case(name: str):
    """(forest, X, ref, budget) of CASES[name]: built once per process, read-only."""
    if name not in _cache:
        from euromillioner_amd.models.forest import RandomForest

        depth, T, draws, lags, rows, min_leaf = CASES[name]
        X, Y, F = data(lags)
        rf = RandomForest(n_trees=T, max_depth=depth, min_samples_leaf=min_leaf, seed=11, device="cpu")
        rf.fit(X[:draws], Y[:draws], F)
        Xe = X[:rows].copy()
        if lags == 1:
            Xe = np.concatenate([Xe, np.array([[0], [(1 << 62) - 1]], dtype=np.uint64)])
        ref, bud = shapley_leaves(rf, Xe)
        for a in (Xe, ref, bud):
            a.setflags(write=False)
        _cache[name] = (rf, Xe, ref, bud)
    return _cache[name]
