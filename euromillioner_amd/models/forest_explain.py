"""Explanations of a fitted :class:`~euromillioner_amd.models.forest.RandomForest`: path-dependent TreeSHAP
contributions of ``predict_proba`` and leaf indices (sklearn's ``apply``).

Numpy only, fp64, vectorised over rows and leaves: this module is the ``backend="numpy"`` path and the readable
specification of ``csrc/forest_shap.hip``.

The forest's features are binary.  A split node ``i`` on feature ``f`` sends bit 0 to child ``2i+1`` and bit 1
to child ``2i+2``; a node with ``feat < 0`` reached from the root through ``feat >= 0`` nodes is a leaf and holds
a 62-vector (``value``, padded to 64).  With the stored covers as the background distribution, an unknown
feature averages the two children with ``cover[child] / cover[node]``, the covers in float32 as the device holds
them (this module divides them in fp64, the device in float32).
``predict_proba`` is the mean over the trees, so a tree's contribution is divided by the number of trees.

Contributions use the division-free form of ``gbdt_explain``.  The path of a leaf ``L`` crosses ``d <= max_depth``
features (distinct: :func:`validate` refuses a path that splits twice on one feature; a fitted forest has none,
a split with an empty child is never taken).  Per path feature ``j`` the table keeps the side taken (the bit a row
needs to follow the path) and the zero fraction ``z_j = cover[child] / cover[parent]``.  With ``o_j = 1`` if the
row's bit equals the side and 0 otherwise, the leaf adds

    value[L, o] / T * (o_i - z_i) * sum_{s=0..d-1} s! (d-1-s)! / d! * c_s          to phi[o, f_i],

where ``c_s`` is the coefficient of ``x^s`` in ``prod_{j != i} (z_j + o_j x)``, and ``value[L, o] / T * prod_j z_j``
to the bias.  The weight does not depend on the output ``o``: it is computed once per (row, leaf, path feature)
and applied to the leaf's whole value row.  ``phi[r, o, :F].sum() + phi[r, o, F] == predict_proba[r, o]``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .forest import unpack_bits
from .gbdt_explain import shapley_weights

N_OUT = 62


# ----------------------------------------------------------------------------- validation and the leaf-path table
def leaf_mask(feat: np.ndarray) -> np.ndarray:
    """bool ``[T, nodes]``: the nodes with ``feat < 0`` that the root reaches through ``feat >= 0`` nodes."""
    feat = np.asarray(feat)
    T, NN = feat.shape
    reach = np.zeros((T, NN), dtype=bool)
    reach[:, 0] = True
    for i in range((NN - 1) // 2):
        down = reach[:, i] & (feat[:, i] >= 0)
        reach[:, 2 * i + 1] |= down
        reach[:, 2 * i + 2] |= down
    return reach & (feat < 0)


@dataclass
class PathTable:
    """One entry per leaf, trees ascending then heap slots ascending.  ``d[e]`` path features; columns
    ``j >= d[e]`` of ``feat / side / z`` are padding (feat 0, side 0, z 1)."""
    tree: np.ndarray  # [L] int64
    node: np.ndarray  # [L] int64 heap index of the leaf
    d: np.ndarray  # [L] int64
    feat: np.ndarray  # [L, D] int64
    side: np.ndarray  # [L, D] int64: the bit a row needs at feat to follow the path
    z: np.ndarray  # [L, D] float64 quotients of the float32 covers
    value: np.ndarray  # [L, 64] float64
    n_trees: int


def validate(feat, cover, F: int, max_depth: int) -> None:
    """Raise ``ValueError`` unless the forest is a set of well-formed heap trees over ``F`` binary features:
    ``feat`` in ``[-2, F)``, no reachable split at the last level, every reachable split with ``cover > 0``,
    and no path that splits twice on one feature."""
    feat, cover = np.asarray(feat), np.asarray(cover)
    if feat.ndim != 2 or feat.shape[1] != 2 ** (max_depth + 1) - 1 or cover.shape != feat.shape:
        raise ValueError(f"feat / cover must be [T, {2 ** (max_depth + 1) - 1}] for max_depth {max_depth}")
    bad = (feat < -2) | (feat >= int(F))
    if bad.any():
        t, i = (int(v[0]) for v in np.nonzero(bad))
        raise ValueError(f"tree {t} node {i} has feat {int(feat[t, i])}, outside [-2, {F})")
    T, NN = feat.shape
    reach = np.zeros((T, NN), dtype=bool)
    reach[:, 0] = True
    seen = np.zeros((T, NN, max(1, (int(F) + 63) // 64)), dtype=np.uint64)  # features split on above each node
    for i in range(NN):
        split = reach[:, i] & (feat[:, i] >= 0)
        if not split.any():
            continue
        t = np.nonzero(split)[0]
        if 2 * i + 2 >= NN:
            raise ValueError(f"tree {int(t[0])} node {i} is a split at the last level (children out of range)")
        cv = cover[t, i]
        if not (cv > 0).all():  # also catches NaN
            k = int(np.nonzero(~(cv > 0))[0][0])
            raise ValueError(f"tree {int(t[k])} node {i} is a split with cover {float(cv[k])} (must be > 0)")
        f = feat[t, i].astype(np.int64)
        w, b = f >> 6, np.uint64(1) << (f & 63).astype(np.uint64)
        twice = (seen[t, i, w] & b) != 0
        if twice.any():
            k = int(np.nonzero(twice)[0][0])
            raise ValueError(f"tree {int(t[k])} node {i} splits on feature {int(f[k])} a second time on its path")
        for c in (2 * i + 1, 2 * i + 2):
            reach[t, c] = True
            seen[t, c] = seen[t, i]
            seen[t, c, w] |= b


def build_paths(feat, value, cover, max_depth: int) -> PathTable:
    """The leaf-path table of a validated forest (module docstring)."""
    feat, value = np.asarray(feat), np.asarray(value)
    cover = np.asarray(cover, dtype=np.float32)
    D = max(1, int(max_depth))
    tree, node = np.nonzero(leaf_mask(feat))
    L = len(tree)
    depth = np.frexp(node + 1.0)[1].astype(np.int64) - 1  # bit_length(node + 1) - 1, exact
    pf, ps, pz = np.zeros((L, D), np.int64), np.zeros((L, D), np.int64), np.ones((L, D))
    for lvl in range(int(max_depth)):
        on = depth > lvl
        sh = np.where(on, depth - lvl, 0)
        p = ((node + 1) >> sh) - 1
        c = ((node + 1) >> np.maximum(sh - 1, 0)) - 1
        pf[on, lvl] = feat[tree[on], p[on]]
        ps[on, lvl] = c[on] - (2 * p[on] + 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            pz[on, lvl] = cover[tree[on], c[on]].astype(np.float64) / cover[tree[on], p[on]].astype(np.float64)
    return PathTable(tree.astype(np.int64), node.astype(np.int64), depth, pf, ps, pz,
                     value[tree, node].astype(np.float64), int(feat.shape[0]))


# ----------------------------------------------------------------------------- contributions
def contribs_from_paths(paths: PathTable, bits: np.ndarray, leaf_chunk: int | None = None) -> np.ndarray:
    """float64 ``[n, 62, F+1]`` from a path table and the rows' feature bits ``[n, F]`` (bias in the last column)."""
    bits = np.asarray(bits).astype(np.int64)
    n, F = bits.shape
    T = max(paths.n_trees, 1)
    phi = np.zeros((F + 1, n, N_OUT))  # [column, row, output]: a leaf adds a rank-one [row] x [output] block
    V = paths.value[:, :N_OUT] / T
    bias = (V * np.prod(paths.z, axis=1)[:, None]).sum(axis=0)
    phi[F] = bias[None, :]
    chunk = leaf_chunk or max(1, (1 << 21) // max(n, 1))
    for d in range(1, paths.feat.shape[1] + 1):
        sel = np.nonzero(paths.d == d)[0]
        w = shapley_weights(d)
        for a in range(0, len(sel), chunk):
            e = sel[a:a + chunk]
            f, z = paths.feat[e, :d], paths.z[e, :d]  # [L, d]
            o = (bits[:, f] == paths.side[e, :d]).astype(np.float64)  # [n, L, d]
            for i in range(d):
                c = np.zeros((d,) + o.shape[:2])  # coefficients of prod_{j != i} (z_j + o_j x)
                c[0] = 1.0
                deg = 0
                for j in range(d):
                    if j == i:
                        continue
                    c[1:deg + 2] = c[1:deg + 2] * z[:, j] + c[0:deg + 1] * o[:, :, j]
                    c[0] = c[0] * z[:, j]
                    deg += 1
                s = (o[:, :, i] - z[:, i]) * np.tensordot(w, c, axes=1)  # [n, L]
                fi = f[:, i]
                for g in np.unique(fi):
                    m = fi == g
                    phi[g] += s[:, m] @ V[e[m]]
    return np.ascontiguousarray(phi.transpose(1, 2, 0))


def row_bits(rf, X) -> np.ndarray:
    X = np.asarray(X, dtype=np.uint64).reshape(len(X), -1)
    if X.shape[1] * 64 < rf.F:
        raise ValueError(f"X has {X.shape[1]} feature words, the forest needs {(rf.F + 63) // 64}")
    return unpack_bits(X, rf.F)


def paths_of(rf) -> PathTable:
    """The validated path table of a forest, cached on it (keyed by its ``feat`` array)."""
    cached = getattr(rf, "_explain_paths", None)
    if cached is not None and cached[0] is rf.feat:
        return cached[1]
    if rf.feat is None:
        raise ValueError("the forest is not fitted")
    validate(rf.feat, rf.cover, rf.F, rf.max_depth)
    paths = build_paths(rf.feat, rf.value, rf.cover, rf.max_depth)
    rf._explain_paths = (rf.feat, paths)
    return paths


def contribs_numpy(rf, X) -> np.ndarray:
    """float64 ``[n, 62, F+1]`` TreeSHAP contributions of ``rf.predict_proba`` on packed rows ``X``."""
    return contribs_from_paths(paths_of(rf), row_bits(rf, X))


# ----------------------------------------------------------------------------- leaf indices
def apply_numpy(rf, X) -> np.ndarray:
    """int32 ``[n, T]``: the heap index of the node where each row's walk stops in each tree."""
    paths_of(rf)  # (validation)
    bits = row_bits(rf, X)
    n, T = len(bits), len(rf.feat)
    out = np.zeros((n, T), dtype=np.int32)
    rows = np.arange(n)
    for t in range(T):
        node = np.zeros(n, dtype=np.int64)
        while True:
            f = rf.feat[t][node]
            act = f >= 0
            if not act.any():
                break
            node[act] = 2 * node[act] + 1 + bits[rows[act], f[act]]
        out[:, t] = node
    return out


# ----------------------------------------------------------------------------- names
def feature_names(F: int) -> list[str]:
    """Names of the forest's input columns in the ``lag_features`` layout: block ``k`` of 62 is draw
    ``t - lags + 1 + k``, so the last block is the latest draw (lag 1)."""
    lags = max(1, F // 62)
    one = [f"number {i + 1}" for i in range(50)] + [f"star {i + 1}" for i in range(12)]
    if lags == 1:
        return (one + [f"f{i}" for i in range(62, F)])[:F]
    names = [f"{nm} (lag {lags - k})" for k in range(lags) for nm in one]
    return (names + [f"f{i}" for i in range(len(names), F)])[:F]
