"""A per-node check of a fitted random forest, from the definition (numpy, fp64 and exact integers).

:func:`check_forest` takes the four arrays of a fitted forest (either engine's), its training rows and the fit's
parameters, and checks every node of every tree.  It regrows nothing and does not import the numpy engine
(``models/forest_oracle.py``): from ``models/forest.py`` it takes only the two hashes that ARE the specification,
``poisson_weights`` (the bootstrap weight of (seed, tree, row)) and ``candidates`` (the candidate features of (seed,
tree, node)).  The packed ``X`` words are read directly.

Walk.  Per tree, from the root ALONG THE FOREST'S OWN SPLITS: the rows that reach a child are its parent's rows
whose split bit is 0 (left, node 2i + 1) or 1 (right, 2i + 2), so what is checked at a node never depends on a
decision the reference would have taken differently above it.  The root holds the rows of weight > 0.  The first
offending (tree, node) raises :class:`ForestMismatch`, which names the tree, the node and the field.

At every reached node, with w the weights, n = sum w and S_j = sum w y_j (integers):

* ``cover == float32(n)``;
* ``value[:62] == float32(float64(S_j) / float64(n))`` bit for bit and ``value[62:] == 0`` (integer sums and one
  correctly rounded division are reproducible: no tolerance); all zero when n == 0.

Leaf or split.  A node may split iff ``level < max_depth`` and ``n >= 2 * min_leaf``.  Over its candidates f in
ascending order with ``nL, nR >= max(min_leaf, 1)`` (nR = sum w x_f) the gain is the fp64 expression

    float(aL) / float(nL) + float(aR) / float(nR) - float(s2) / float(n)

of the exact integers aL = sum_j SL_j^2, aR = sum_j SR_j^2, s2 = sum_j S_j^2.  The winner is the largest gain, the
lowest feature index on a tie, and it is kept iff ``g > 1e-9 * (1 + g)``.  ``feat`` must equal the winner (-1 if
none) and ``gain`` its value bit for bit (0.0 if none).

Exact cross-check of the fp64 rule.  In integers, the chosen split's exact gain must reach the exact maximum over
the admissible candidates minus ``2^-50 * (aL/nL + aR/nR + s2/n)`` of the chosen split.  Derivation: the fp64
expression has five roundings (three divisions, one sum, one difference) of at most 2^-53 relative each, on
magnitudes no larger than that sum, so a computed gain is within 5 * 2^-53 of the sum of its exact value; the
rounded ``s2 / n`` is the same number for every candidate of the node and cancels in a comparison, which leaves at
most 3 * 2^-53 per candidate and 6 * 2^-53 < 2^-50 for the pair (the larger fp64 gain has, to that precision, the
larger sum).  Every integer the expression converts is below 2^53 (asserted), so the conversions are exact.

Unreached nodes (under a leaf or under an unreached node): ``feat == -2`` and ``gain == 0``.  A reached node at
``max_depth`` is a leaf: ``feat == -1``, ``gain == 0``.

The sums are float64 matrix products of non-negative integers whose every partial sum is an integer below 2^53:
exact in any order.  Squares and the cross-check run on int64 / Python integers.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from euromillioner_amd.models.forest import candidates, poisson_weights


class ForestMismatch(AssertionError):
    def __init__(self, tree: int, node: int, fld: str, detail: str):
        self.tree, self.node, self.field = int(tree), int(node), fld
        super().__init__(f"tree {tree} node {node}: {fld}: {detail}")


@dataclass
class Report:
    """Per level: reached nodes, the largest distinct-row count of a node (rows of weight > 0: what the device's
    segments count) and the largest flat index ``t * 2^level + nd`` (t: position in ``trees``) of a reached node."""
    reached: list = field(default_factory=list)
    max_rows: list = field(default_factory=list)
    max_flat: list = field(default_factory=list)
    nodes: int = 0
    splits: int = 0


def _f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f64_bits(x) -> int:
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def _exact_guard(t, node, ci, aL, aR, nL, nR, s2, n, ok):
    """The chosen candidate ci against every admissible one, in Python integers (see the module docstring)."""
    o = lambda a: a.astype(object)  # noqa: E731
    aL, aR, nL, nR = o(aL), o(aR), o(nL), o(nR)
    s2, n = int(s2), int(n)
    den = nL * nR * n  # > 0 wherever ok
    num = aL * nR * n + aR * nL * n - s2 * nL * nR  # exact gain = num / den
    slack = aL[ci] * nR[ci] * n + aR[ci] * nL[ci] * n + s2 * nL[ci] * nR[ci]  # (aL/nL + aR/nR + s2/n) * den[ci]
    lhs = (num[ci] << 50) + slack
    for i in np.nonzero(ok)[0]:
        if lhs * den[i] < (num[i] << 50) * den[ci]:
            raise ForestMismatch(t, node, "feat", f"exact gain of the split is below candidate slot {i}'s by more "
                                 f"than the fp64 rule's rounding bound")


def check_forest(X, Y, F, feat, value, gain, cover, trees, max_depth, k, min_leaf, bootstrap, seed) -> Report:
    X = np.ascontiguousarray(np.asarray(X, dtype=np.uint64).reshape(len(X), -1))
    Y = np.asarray(Y, dtype=np.uint64).reshape(-1)
    feat, value, gain, cover = (np.asarray(a) for a in (feat, value, gain, cover))
    trees = list(trees)
    N, T, nodes = len(X), len(trees), (1 << (max_depth + 1)) - 1
    assert len(Y) == N and 9 * N * 9 * N * 62 < 2 ** 53, "row count outside the exact range of this check"
    assert feat.shape == (T, nodes) and value.shape == (T, nodes, 64), (feat.shape, value.shape)
    assert gain.shape == (T, nodes) and cover.shape == (T, nodes), (gain.shape, cover.shape)
    assert value.dtype == np.float32 and cover.dtype == np.float32 and gain.dtype == np.float64
    yb = ((Y[:, None] >> np.arange(62, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64)  # [N, 62]
    min_lr = max(int(min_leaf), 1)
    rep = Report(reached=[0] * (max_depth + 1), max_rows=[0] * (max_depth + 1), max_flat=[-1] * (max_depth + 1))
    gain_bits = np.ascontiguousarray(gain).view(np.uint64)
    for ti, t in enumerate(trees):
        w = poisson_weights(seed, t, N).astype(np.float64) if bootstrap else np.ones(N, dtype=np.float64)
        frontier = {0: np.nonzero(w > 0)[0]}
        reached = np.zeros(nodes, dtype=bool)
        for level in range(max_depth + 1):
            nxt = {}
            for node, rows in frontier.items():
                reached[node] = True
                nd = node - ((1 << level) - 1)
                rep.reached[level] += 1
                rep.max_rows[level] = max(rep.max_rows[level], len(rows))
                rep.max_flat[level] = max(rep.max_flat[level], ti * (1 << level) + nd)
                rep.nodes += 1
                wr = w[rows]
                wy = yb[rows] * wr[:, None]
                S = np.rint(wy.sum(0)).astype(np.int64)  # [62]
                n = int(round(float(wr.sum())))
                # ---- node record
                if _f32_bits(cover[ti, node]) != _f32_bits(np.float32(n)):
                    raise ForestMismatch(t, node, "cover", f"{cover[ti, node]!r} != {float(n)!r}")
                want = np.zeros(64, dtype=np.float32)
                if n > 0:
                    want[:62] = (S.astype(np.float64) / np.float64(n)).astype(np.float32)
                bad = np.nonzero(_f32_bits(value[ti, node]) != _f32_bits(want))[0]
                if len(bad):
                    j = int(bad[0])
                    raise ForestMismatch(t, node, "value", f"output {j}: {value[ti, node, j]!r} != {want[j]!r}")
                # ---- leaf or split, from the definition
                f_best, g_best, ci, parts = -1, 0.0, -1, None
                if level < max_depth and n >= 2 * min_leaf and n > 0:
                    cs = np.sort(candidates(seed, t, node, F, k))
                    xc = ((X[rows[:, None], (cs >> 6)[None, :]] >> (cs & 63).astype(np.uint64)[None, :])
                          & np.uint64(1)).astype(np.float64)  # [rows, k]
                    nR = np.rint(xc.T @ wr).astype(np.int64)
                    SR = np.rint(xc.T @ wy).astype(np.int64)  # [k, 62]
                    nL, SL = n - nR, S[None, :] - SR
                    aL, aR, s2 = (SL * SL).sum(1), (SR * SR).sum(1), int((S * S).sum())
                    ok = (nL >= min_lr) & (nR >= min_lr)
                    if ok.any():
                        with np.errstate(divide="ignore", invalid="ignore"):
                            g = (aL.astype(np.float64) / nL.astype(np.float64)
                                 + aR.astype(np.float64) / nR.astype(np.float64)) - np.float64(s2) / np.float64(n)
                        g = np.where(ok, g, -np.inf)
                        ci = int(np.argmax(g))  # first maximum = lowest feature index
                        gb = float(g[ci])
                        if gb > 1e-9 * (1.0 + gb):
                            f_best, g_best = int(cs[ci]), gb
                        parts = (cs, aL, aR, nL, nR, s2, ok)
                f_dev = int(feat[ti, node])
                if f_dev != f_best:
                    raise ForestMismatch(t, node, "feat", f"{f_dev} != {f_best} (reference gain {g_best!r})")
                if int(gain_bits[ti, node]) != _f64_bits(g_best):
                    raise ForestMismatch(t, node, "gain", f"{float(gain[ti, node])!r} != {g_best!r}")
                if f_best >= 0:
                    cs, aL, aR, nL, nR, s2, ok = parts
                    _exact_guard(t, node, ci, aL, aR, nL, nR, s2, n, ok)
                    rep.splits += 1
                    right = ((X[rows, f_best >> 6] >> np.uint64(f_best & 63)) & np.uint64(1)).astype(bool)
                    nxt[2 * node + 1] = rows[~right]
                    nxt[2 * node + 2] = rows[right]
            frontier = nxt
        for node in np.nonzero(~reached)[0]:
            if int(feat[ti, node]) != -2:
                raise ForestMismatch(t, node, "feat", f"unreached node has {int(feat[ti, node])}, not -2")
            if int(gain_bits[ti, node]) != 0:
                raise ForestMismatch(t, node, "gain", f"unreached node has {float(gain[ti, node])!r}, not 0.0")
    return rep
