"""The yardstick of the GBDT contributions (``GBDT.predict_contribs``): fp64 Shapley values straight from the
definition, and the error budget of a float32 engine.

Numpy only, and independent of the leaf-path table of ``euromillioner_amd/models/gbdt_explain.py``.

Reference.  :func:`shapley` takes, per tree, the set ``U`` of features the tree splits on and computes the
value ``v(S)`` of every subset ``S`` of ``U`` with the cover-weighted recursion: at a split on a feature in
``S`` follow the row (right iff ``bin > sbin``), otherwise average the two children with
``cover[child] / cover[parent]`` (the stored covers; they need not add up).  Then

    phi_j = sum over S in U \\ {j} of |S|! (|U| - |S| - 1)! / |U|! * (v(S + j) - v(S)),     bias = v({}),

tree ``k`` is credited to task ``k % T`` and the bias gets ``base_margin`` once.  Bins come from
``_gbdt_ref.bin_features``; the tree arrays are taken as the model holds them.

Budget.  :func:`budget` is the largest ``|engine - reference|`` allowed per output element, computed from the
reference's own values only.  Error model, with ``u = 2^-24`` and ``g(k) = k u / (1 - k u)`` the standard bound on
``k`` accumulated roundings.  The inputs (float32 leaves, the covers rounded to float32, integer bins) are the same on
both sides.  An engine evaluates, per leaf whose path crosses ``d <= D`` distinct features (``D`` = max_depth),

    term_i = leaf * (o_i - z_i) * sum_s w_s c_s,      c = coefficients of prod_{j != i} (z_j + o_j x)

in float32 and adds the terms of an output element in float32, ``N`` of them.  Let ``A`` be the same sum as the
reference's with every term replaced by its absolute value (``o_i - z_i -> o_i + z_i``; everything else is
non-negative).  Counting roundings of one term, each relative to the term's magnitude:

* the ``z_j``: a path has at most ``D`` edges, each edge one division, and the ``z`` of a feature met ``m``
  times ``m - 1`` multiplications: at most ``2 D`` roundings over ALL ``z`` of a path together;
* the ``c_s``: ``d - 1`` factors multiplied into the polynomial, each step one product and one add (or one fused
  multiply-add and one product) per coefficient, all operands non-negative, so no cancellation:
  at most ``2 (D - 1)``;
* ``sum_s w_s c_s``: the rounding of ``w_s``, the product, ``d - 1`` additions of non-negative values:
  at most ``D + 1``;
* ``o_i - z_i`` (its rounding error is at most ``u (o_i + z_i)``), times ``leaf``, times the sum: 3.

That is ``5 D + 2`` roundings per term, and the float32 accumulation of ``N`` terms adds ``N - 1`` (for the bias
column, which also adds ``base_margin``, ``N`` is the number of leaves plus one).  Storing as float32 is covered
by a last ``2^-23 |ref|``.  Hence

    budget = g(N + 5 D + 2) * A + 2^-23 * |ref|.

``N`` is counted per output column: the leaves of the task's trees whose path crosses the feature.  A column no
tree of the task splits on has ``A = 0``, ``ref = 0`` and budget 0: it must be exactly 0.  The constant comes from
this count, not from any engine's error.
"""
from __future__ import annotations

import math

import numpy as np

import _gbdt_ref as R

U32 = 2.0 ** -24


def round_covers(trees) -> None:
    """Round the model's covers to float32 in place: the values a device engine holds (a HIP fit already does)."""
    trees.cover[...] = np.asarray(trees.cover, np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- Shapley values by definition
def _tree_values(status, feat, sbin, leaf, cover, bins, U):
    """v[S, r] for every subset S of U (bit j of S <-> U[j]) and row r."""
    m, n = len(U), bins.shape[0]
    pos = {f: j for j, f in enumerate(U)}
    S = np.arange(1 << m)

    def rec(i):
        if status[i] != 1:
            return np.full((len(S), n), float(leaf[i]))
        l, r = 2 * i + 1, 2 * i + 2
        vl, vr = rec(l), rec(r)
        f = int(feat[i])
        known = ((S >> pos[f]) & 1).astype(bool)[:, None]
        right = (bins[:, f] > sbin[i])[None, :]
        follow = np.where(right, vr, vl)
        mean = (float(cover[l]) / float(cover[i])) * vl + (float(cover[r]) / float(cover[i])) * vr
        return np.where(known, follow, mean)

    return rec(0)


def _reachable_splits(status):
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        if status[i] == 1:
            out.append(i)
            stack += [2 * i + 1, 2 * i + 2]
    return out


def shapley(trees, sbin, bins, n_tasks: int, base_margin: float, k0: int = 0, k1: int | None = None) -> np.ndarray:
    """fp64 ``[n, T, F+1]`` Shapley values of the trees ``[k0, k1)`` on binned rows (module docstring)."""
    bins = np.asarray(bins, np.int64)
    n, F = bins.shape
    T = int(n_tasks)
    K = trees.status.shape[0]
    k1 = K if k1 is None else k1
    out = np.zeros((n, T, F + 1))
    out[:, :, F] = base_margin
    for k in range(k0, k1):
        st, ft = trees.status[k], trees.feat[k]
        U = sorted({int(ft[i]) for i in _reachable_splits(st)})
        m = len(U)
        v = _tree_values(st, ft, sbin[k], trees.leaf[k], trees.cover[k], bins, U)
        t = k % T
        out[:, t, F] += v[0]
        S = np.arange(1 << m)
        size = np.array([bin(int(s)).count("1") for s in S])
        for j, f in enumerate(U):
            without = S[((S >> j) & 1) == 0]
            w = np.array([math.factorial(int(c)) * math.factorial(m - int(c) - 1) / math.factorial(m)
                          for c in size[without]])
            out[:, t, f] += (w[:, None] * (v[without | (1 << j)] - v[without])).sum(axis=0)
    return out


# ----------------------------------------------------------------------------- the budget
def _leaf_paths(status, feat, sbin, cover):
    """[(leaf node, {feature: [lo, hi, z]})] of one tree, by descending from the root."""
    out = []

    def go(i, path):
        if status[i] != 1:
            out.append((i, path))
            return
        f, b = int(feat[i]), int(sbin[i])
        for c, right in ((2 * i + 1, False), (2 * i + 2, True)):
            p = {g: list(v) for g, v in path.items()}
            lo, hi, z = p.get(f, [-1, np.inf, 1.0])
            if right:
                lo = max(lo, b)
            else:
                hi = min(hi, b)
            p[f] = [lo, hi, z * float(cover[c]) / float(cover[i])]
            go(c, p)

    go(0, {})
    return out


def magnitudes(trees, sbin, bins, n_tasks: int, base_margin: float, k0: int = 0, k1: int | None = None):
    """``(A [n, T, F+1], N [T, F+1])`` of the module docstring: the sums of the absolute values of the terms an
    engine accumulates, and how many terms each output column accumulates."""
    bins = np.asarray(bins, np.int64)
    n, F = bins.shape
    T = int(n_tasks)
    K = trees.status.shape[0]
    k1 = K if k1 is None else k1
    A = np.zeros((n, T, F + 1))
    N = np.zeros((T, F + 1), dtype=np.int64)
    A[:, :, F] = abs(base_margin)
    N[:, F] = 1
    for k in range(k0, k1):
        t = k % T
        for i, path in _leaf_paths(trees.status[k], trees.feat[k], sbin[k], trees.cover[k]):
            lv = abs(float(trees.leaf[k, i]))
            fs = list(path)
            d = len(fs)
            z = [path[f][2] for f in fs]
            o = [((bins[:, f] > path[f][0]) & (bins[:, f] <= path[f][1])).astype(np.float64) for f in fs]
            A[:, t, F] += lv * float(np.prod(z)) if d else lv
            N[t, F] += 1
            for a, f in enumerate(fs):
                c = [np.ones(n)] + [np.zeros(n) for _ in range(d - 1)]
                deg = 0
                for j in range(d):
                    if j == a:
                        continue
                    for s in range(deg + 1, 0, -1):
                        c[s] = c[s] * z[j] + c[s - 1] * o[j]
                    c[0] = c[0] * z[j]
                    deg += 1
                tot = sum(math.factorial(s) * math.factorial(d - 1 - s) / math.factorial(d) * c[s] for s in range(d))
                A[:, t, f] += lv * (o[a] + z[a]) * tot
                N[t, f] += 1
    return A, N


def budget(ref: np.ndarray, A: np.ndarray, N: np.ndarray, max_depth: int) -> np.ndarray:
    """Largest allowed ``|engine - ref|`` per element of ``ref [n, T, F+1]`` (module docstring)."""
    k = (N + 5 * int(max_depth) + 2).astype(np.float64) * U32
    return (k / (1.0 - k))[None, :, :] * A + 2.0 ** -23 * np.abs(ref)


def reference(model, X, iteration_range=None):
    """``(ref, budget)``, both fp64 ``[n, T, F+1]``, from the model's own trees and cuts."""
    tr = model.trees
    T = model.n_tasks
    bins = R.bin_features(X, model.cuts)
    k0, k1 = (0, tr.n_trees) if iteration_range is None else (iteration_range[0] * T, iteration_range[1] * T)
    ref = shapley(tr, tr.sbin, bins, T, model.base_margin, k0, k1)
    A, N = magnitudes(tr, tr.sbin, bins, T, model.base_margin, k0, k1)
    return ref, budget(ref, A, N, tr.max_depth)


def worst_ratio(dev, ref, bud) -> float:
    """max |dev - ref| / budget over the elements with a non-zero budget."""
    err = np.abs(np.asarray(dev, np.float64) - ref)
    nz = bud > 0
    return float((err[nz] / bud[nz]).max()) if nz.any() else 0.0


def violations(dev, ref, bud) -> int:
    dev = np.asarray(dev, np.float64)
    return int((~np.isfinite(dev) | (np.abs(dev - ref) > bud)).sum())


# ----------------------------------------------------------------------------- plain walks
def heap_walk(trees, sbin, bins) -> np.ndarray:
    """int [n, K]: where each row stops in each tree, one row and one tree at a time."""
    n, K = bins.shape[0], trees.status.shape[0]
    out = np.zeros((n, K), dtype=np.int64)
    for k in range(K):
        for r in range(n):
            i = 0
            while trees.status[k, i] == 1:
                i = 2 * i + 1 + int(bins[r, trees.feat[k, i]] > sbin[k, i])
            out[r, k] = i
    return out
