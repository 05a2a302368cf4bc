"""Explanations of a fitted :class:`~euromillioner_amd.models.gbdt.GBDT`: path-dependent TreeSHAP contributions
(XGBoost's ``pred_contribs``), leaf indices (``pred_leaf``) and feature importances (``get_score``).

Numpy only, fp64, vectorised over rows: this module is the ``backend="numpy"`` path and the readable
specification of ``csrc/gbdt_shap.hip``.

Contributions use a division-free form of path-dependent TreeSHAP.  For each leaf ``L`` of a tree, the path
from the root crosses ``d <= max_depth`` distinct features.  For each such feature ``j`` the path keeps

* a bin interval ``(lo_j, hi_j]``: a row follows every split on ``j`` along the path iff
  ``lo_j < bin[j] <= hi_j`` (the engines go right iff ``bin > sbin``: a left edge sets ``hi = min(hi, sbin)``,
  a right edge ``lo = max(lo, sbin)``; repeated splits on one feature intersect);
* a zero fraction ``z_j``: the product, over the path's edges that split on ``j``, of
  ``cover[child] / cover[parent]`` (the stored covers, as XGBoost uses them).

With ``o_j = 1`` if the row is inside the interval of ``j`` and 0 otherwise, the leaf adds

    leaf * (o_i - z_i) * sum_{s=0..d-1} s! (d-1-s)! / d! * c_s          to phi[f_i],

where ``c_s`` is the coefficient of ``x^s`` in ``prod_{j != i} (z_j + o_j x)``, and ``leaf * prod_j z_j`` to the
bias.  A leaf at the root (``d = 0``) adds its value to the bias only.  Tree ``k`` belongs to task ``k % T`` and
the bias also gets ``base_margin`` once, so ``sum(phi) + bias == predict_margin``.

Bins.  A fitted model has its cuts and ``sbin``; a loaded checkpoint has ``split_value`` only.  For those
:func:`model_bins` derives both: the cuts of a feature are its sorted unique split values and ``sbin`` the
value's index, so that with ``bin = #cuts <= x`` the test ``bin > sbin`` is ``not (x < split_value)`` exactly.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .gbdt import TreeArrays, apply_bins

IMPORTANCE_TYPES = ("weight", "gain", "cover", "total_gain", "total_cover")
HI_OPEN = np.iinfo(np.int32).max  # "no upper bound yet" of a path interval


# ----------------------------------------------------------------------------- validation and bins
def validate_trees(trees: TreeArrays, num_feature: int) -> None:
    """Raise ``ValueError`` unless every tree is a well-formed heap tree over ``num_feature`` features: the root
    is used, every split has ``0 <= feat < F``, ``cover > 0`` and two used children inside the array, and every
    used node below the root hangs under a split."""
    st = np.asarray(trees.status)
    K, NN = st.shape
    if NN != 2 ** (trees.max_depth + 1) - 1:
        raise ValueError(f"trees have {NN} node slots, max_depth {trees.max_depth} needs {2 ** (trees.max_depth + 1) - 1}")
    if K and (st[:, 0] == 0).any():
        raise ValueError(f"tree {int(np.nonzero(st[:, 0] == 0)[0][0])} has no root")
    if ((st < 0) | (st > 2)).any():
        raise ValueError("node status must be 0 (unused), 1 (split) or 2 (leaf)")
    k, i = np.nonzero(st == 1)
    if k.size:
        f = np.asarray(trees.feat)[k, i]
        bad = (f < 0) | (f >= int(num_feature))
        if bad.any():
            j = int(np.nonzero(bad)[0][0])
            raise ValueError(f"tree {int(k[j])} node {int(i[j])} splits on feature {int(f[j])}, outside [0, {num_feature})")
        deep = 2 * i + 2 >= NN
        if deep.any():
            j = int(np.nonzero(deep)[0][0])
            raise ValueError(f"tree {int(k[j])} node {int(i[j])} is a split at the last level (children out of range)")
        gone = (st[k, 2 * i + 1] == 0) | (st[k, 2 * i + 2] == 0)
        if gone.any():
            j = int(np.nonzero(gone)[0][0])
            raise ValueError(f"tree {int(k[j])} node {int(i[j])} is a split with a missing child")
        cv = np.asarray(trees.cover)[k, i]
        if not (cv > 0).all():  # also catches NaN
            j = int(np.nonzero(~(cv > 0))[0][0])
            raise ValueError(f"tree {int(k[j])} node {int(i[j])} is a split with cover {float(cv[j])} (must be > 0)")
    k, i = np.nonzero(st[:, 1:])
    if k.size:
        i = i + 1
        orphan = st[k, (i - 1) // 2] != 1
        if orphan.any():
            j = int(np.nonzero(orphan)[0][0])
            raise ValueError(f"tree {int(k[j])} node {int(i[j])} is used but its parent is not a split")


def num_features(model) -> int:
    if model.cuts is not None:
        return len(model.cuts)
    if model.num_feature is not None:
        return int(model.num_feature)
    raise ValueError("the model does not know its number of features")


def model_bins(model):
    """``(cuts, sbin)`` for routing on bins: the model's own after ``fit``, derived from ``split_value`` for a
    loaded checkpoint (module docstring).  The derived pair is cached on the model."""
    if model.cuts is not None:
        return model.cuts, model.trees.sbin
    cached = getattr(model, "_explain_bins", None)
    if cached is not None:
        return cached
    tr = model.trees
    F = num_features(model)
    validate_trees(tr, F)
    k, i = np.nonzero(tr.status == 1)
    f, v = tr.feat[k, i], tr.split_value[k, i]
    cuts = [np.unique(v[f == j]) for j in range(F)]
    sbin = np.zeros(tr.feat.shape, dtype=np.int32)
    for j in range(F):
        m = f == j
        if m.any():
            sbin[k[m], i[m]] = np.searchsorted(cuts[j], v[m])
    model._explain_bins = (cuts, sbin)
    return cuts, sbin


# ----------------------------------------------------------------------------- the leaf-path table
@dataclass
class PathTable:
    """One entry per leaf, trees ascending then heap slots ascending.  ``d[e]`` distinct features; columns
    ``j >= d[e]`` of ``feat / lo / hi / z`` are padding (feat -1, z 1)."""
    tree: np.ndarray  # [L] int64
    node: np.ndarray  # [L] int64 heap index of the leaf
    d: np.ndarray  # [L] int64
    leaf: np.ndarray  # [L] float64
    feat: np.ndarray  # [L, D] int64
    lo: np.ndarray  # [L, D] int64
    hi: np.ndarray  # [L, D] int64
    z: np.ndarray  # [L, D] float64
    bias: np.ndarray  # [L] float64: leaf * prod_j z_j


def build_paths(status, feat, sbin, leaf, cover, max_depth: int, k0: int = 0, k1: int | None = None) -> PathTable:
    """The leaf-path table of trees ``[k0, k1)`` (module docstring)."""
    status = np.asarray(status)
    K = status.shape[0]
    k1 = K if k1 is None else k1
    D = max(1, int(max_depth))
    rows = []
    for k in range(k0, k1):
        for i in np.nonzero(status[k] == 2)[0]:
            i = int(i)
            depth = (i + 1).bit_length() - 1
            fs, lo, hi, z = [], [], [], []
            for lvl in range(depth):
                p = ((i + 1) >> (depth - lvl)) - 1
                c = ((i + 1) >> (depth - lvl - 1)) - 1
                f, b = int(feat[k, p]), int(sbin[k, p])
                if f in fs:
                    j = fs.index(f)
                else:
                    j = len(fs)
                    fs.append(f), lo.append(-1), hi.append(HI_OPEN), z.append(1.0)
                if c == 2 * p + 2:
                    lo[j] = max(lo[j], b)
                else:
                    hi[j] = min(hi[j], b)
                z[j] *= float(cover[k, c]) / float(cover[k, p])
            rows.append((k, i, fs, lo, hi, z, float(leaf[k, i])))
    L = len(rows)
    t = PathTable(np.zeros(L, np.int64), np.zeros(L, np.int64), np.zeros(L, np.int64), np.zeros(L),
                  np.full((L, D), -1, np.int64), np.full((L, D), -1, np.int64), np.full((L, D), HI_OPEN, np.int64),
                  np.ones((L, D)), np.zeros(L))
    for e, (k, i, fs, lo, hi, z, lv) in enumerate(rows):
        d = len(fs)
        t.tree[e], t.node[e], t.d[e], t.leaf[e] = k, i, d, lv
        t.feat[e, :d], t.lo[e, :d], t.hi[e, :d], t.z[e, :d] = fs, lo, hi, z
        t.bias[e] = lv * float(np.prod(z)) if d else lv
    return t


def shapley_weights(d: int) -> np.ndarray:
    """``s! (d-1-s)! / d!`` for s = 0..d-1."""
    return np.array([math.factorial(s) * math.factorial(d - 1 - s) / math.factorial(d) for s in range(d)])


# ----------------------------------------------------------------------------- contributions
def contribs_from_paths(paths: PathTable, bins: np.ndarray, n_tasks: int, base_margin: float,
                        leaf_chunk: int | None = None) -> np.ndarray:
    """float64 ``[n, T, F+1]`` from a path table and binned rows (the last column is the bias)."""
    bins = np.asarray(bins).astype(np.int64)
    n, F = bins.shape
    T = int(n_tasks)
    phi = np.zeros((T * (F + 1), n))  # [(task, column), row]: leaves scatter-add whole rows
    task = paths.tree % T
    np.add.at(phi, task * (F + 1) + F, paths.bias[:, None])
    phi[np.arange(T) * (F + 1) + F] += base_margin
    chunk = leaf_chunk or max(1, (1 << 21) // max(n, 1))
    for d in range(1, paths.feat.shape[1] + 1):
        sel = np.nonzero(paths.d == d)[0]
        w = shapley_weights(d)
        for a in range(0, len(sel), chunk):
            e = sel[a:a + chunk]
            f, z = paths.feat[e, :d], paths.z[e, :d]  # [L, d]
            b = bins[:, f]  # [n, L, d]
            o = ((b > paths.lo[e, :d]) & (b <= paths.hi[e, :d])).astype(np.float64)
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
                s = np.tensordot(w, c, axes=1)  # [n, L]
                val = paths.leaf[e] * (o[:, :, i] - z[:, i]) * s
                np.add.at(phi, task[e] * (F + 1) + f[:, i], val.T)
    return np.ascontiguousarray(phi.reshape(T, F + 1, n).transpose(2, 0, 1))


def _tree_range(model, iteration_range):
    K, T = model.trees.n_trees, model.n_tasks
    if iteration_range is None:
        return 0, K
    r0, r1 = (int(v) for v in iteration_range)
    if not 0 <= r0 <= r1 <= K // T:
        raise ValueError(f"iteration_range {iteration_range} outside the model's {K // T} rounds")
    return r0 * T, r1 * T


def _bin_rows(model, X):
    cuts, sbin = model_bins(model)
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != len(cuts):
        raise ValueError(f"X must be [n, {len(cuts)}], got {X.shape}")
    return apply_bins(X, cuts), sbin


def contribs_numpy(model, X, iteration_range=None) -> np.ndarray:
    """float64 ``[n, T, F+1]`` TreeSHAP contributions of ``model`` on raw rows ``X``."""
    tr = model.trees
    validate_trees(tr, num_features(model))
    bins, sbin = _bin_rows(model, X)
    k0, k1 = _tree_range(model, iteration_range)
    paths = build_paths(tr.status, tr.feat, sbin, tr.leaf, tr.cover, tr.max_depth, k0, k1)
    return contribs_from_paths(paths, bins, model.n_tasks, model.base_margin)


# ----------------------------------------------------------------------------- leaf indices
def leaf_index_bins(status, feat, sbin, bins: np.ndarray) -> np.ndarray:
    """int32 ``[n, n_trees]``: the heap index of the node where each row's walk stops."""
    status, feat, sbin = np.asarray(status), np.asarray(feat), np.asarray(sbin)
    bins = np.asarray(bins)
    n = bins.shape[0]
    K, NN = status.shape
    out = np.zeros((n, K), dtype=np.int32)
    rows = np.arange(n)
    for k in range(K):
        node = np.zeros(n, dtype=np.int64)
        while True:
            sp = status[k, node] == 1
            if not sp.any():
                break
            nd = node[sp]
            node[sp] = 2 * nd + 1 + (bins[rows[sp], feat[k, nd]] > sbin[k, nd])
        out[:, k] = node
    return out


def leaf_index_numpy(model, X) -> np.ndarray:
    tr = model.trees
    validate_trees(tr, num_features(model))
    bins, sbin = _bin_rows(model, X)
    return leaf_index_bins(tr.status, tr.feat, sbin, bins)


# ----------------------------------------------------------------------------- importances
def importance(trees: TreeArrays, n_tasks: int, num_feature: int, importance_type: str = "weight") -> np.ndarray:
    """float64 ``[T, F]`` with XGBoost's meanings over the split nodes (``status == 1``): ``weight`` the number
    of splits on the feature, ``total_gain`` / ``total_cover`` the sums of the splits' gain / cover, ``gain`` /
    ``cover`` those sums divided by the number of splits (0 where a feature is never used)."""
    if importance_type not in IMPORTANCE_TYPES:
        raise ValueError(f"importance_type must be one of {IMPORTANCE_TYPES}")
    T, F = int(n_tasks), int(num_feature)
    k, i = np.nonzero(trees.status == 1)
    col = (k % T) * F + trees.feat[k, i]
    weight = np.bincount(col, minlength=T * F).astype(np.float64)
    if importance_type == "weight":
        return weight.reshape(T, F)
    src = trees.gain if importance_type.endswith("gain") else trees.cover
    total = np.bincount(col, weights=np.asarray(src, np.float64)[k, i], minlength=T * F)
    if importance_type.startswith("total_"):
        return total.reshape(T, F)
    return np.divide(total, weight, out=np.zeros_like(total), where=weight > 0).reshape(T, F)
