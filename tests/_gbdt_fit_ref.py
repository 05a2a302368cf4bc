"""A plain fp64 regrow of every tree of a fitted GBDT, from the definition (numpy only).

:func:`check_fit` takes a fitted model (either engine's), its training rows and labels, and checks the model
tree by tree from the model's OWN earlier trees: the float32 margins start at ``base_margin`` and, after round r
has been checked, advance with the engine's own trees of that round, ``m = float32(m + float32(leaf))``.  A
failure in round r can therefore neither hide behind nor be caused by a difference in round r - 1.  Nothing here
imports a growing, routing, gradient, quantising or hashing helper of the package; ``tests/_gbdt_ref.py`` gives
the binning rule, the heap walk and the float64 sigmoid / softmax.

Gradients of round r, float64 from the float32 margins and labels:

* logistic: p = sigmoid(m), g = p - y, h = max(p (1 - p), 1e-16);
* squared error: g = m - y, h = 1;
* softmax: g = p - y, h = max(2 p (1 - p), 1e-16).

Subsampling multiplies both by the keep mask of :func:`keep_mask`, written here from the kernel's definition
(``hash3`` in ``csrc/gbdt.hip``): element (round, t, r) is kept iff
``(hash3(seed, uint32(round * 131071 + t), r) >> 8) * 2^-24 < float32(subsample)``, with the absolute round,
``seed & 0xFFFFFFFF`` and, under data parallelism, ``(seed + 0x9E3779B9 * rank) & 0xFFFFFFFF``.

Per-row error bounds (the error model of ``_gbdt_ref.py``: a float32 sigmoid is within 4 ulp, a float32 softmax
probability within (T + 4) 2^-24 relative):

* logistic: |dg|, |dh| <= 2^-21;
* squared error: |dg| <= 2^-24 |g|, dh = 0;
* softmax: |dg| <= (T + 4) 2^-24 p + 2^-25, |dh| <= 2 (T + 4) 2^-24 p + 2^-24;
* fixed-point histograms (``quant_bits_used = s > 0``): + 2^-(s+1) per kept row on dg and + 2^-s on dh (the
  hessian floor rounds a positive h up to one quantum);
* dropped rows contribute nothing;
* both engines add the rows in float64 in some order: the bound of a sum gets 2^-39 of the sum of the absolute
  values on top (n < 2^14 rows, 2^-53 each), which is far below every bound above.

Regrow.  Greedy, in heap order over the bins.  At an open node G, H and their bounds dG, dH are summed over the
node's rows.  Candidate "bin <= b" of feature f (never a feature's last bin) is valid iff HL >= mcw, HR >= mcw,
HL + lambda > 0 and HR + lambda > 0; its gain is GL^2/(HL+l) + GR^2/(HR+l) - G^2/(H+l); the gain's budget is the
corner bound, the largest change of each of the three terms over G +- dG, H +- dH (each term is monotone in |G|
and in H), valid only while H - dH + lambda > 0 (elsewhere the budget is infinite: the candidate, and through
it the node, is ambiguous).  The reference's choice is the first maximum in (feature, bin) order and the node
is split iff that maximum exceeds ``KRT_EPS`` = 1e-6.

Ambiguity, and nothing else, is taken from the engine.  A candidate is SURELY valid when the validity rule
holds at H - dH and POSSIBLY valid when it holds at H + dH.  The engine's split on candidate c is accepted iff c
is possibly valid, gain(c) + budget(c) reaches ``KRT_EPS``, and no surely valid candidate c' has
gain(c') - budget(c') > gain(c) + budget(c): that is "within the two budgets of the reference's best".  If c is
not the reference's own choice the node counts one ambiguous decision and the regrow follows the engine.  Where
the reference's best is within its budget of ``KRT_EPS`` the engine's split or no-split is followed and counted.
After growing to ``max_depth`` the tree is pruned bottom-up: a split whose children are both leaves and whose
gain < gamma becomes a leaf; where |gain - gamma| <= budget + 2^-23 gamma (the engine compares float32 values)
the engine is followed and counted.  A decision the engine is NOT followed on, because it shows none at that
node (a subtree it pruned away), is taken by the reference alone and costs nothing.

Comparison, per tree: ``status`` and ``feat`` equal everywhere, ``sbin`` equal at split nodes, ``leaf`` at
leaves against -G/(H+l) eta (0 where H + l <= 0), ``cover`` against H wherever ``status > 0`` and 0 elsewhere,
``gain`` at split nodes against the candidate's gain; each inside its corner-bound budget + 2^-23 |value| for the
float32 store (which also covers an engine that holds eta in float32); leaves finite.  A pair of columns with
identical bins is named to the checker (``ties``): the sums are bitwise equal on any engine, so no split may use
the higher index, checked exactly and not through the ambiguity rule.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import _gbdt_ref as R

KRT_EPS = 1e-6
STORE = 2.0 ** -23  # float32 store of a result
SUM_SLACK = 2.0 ** -39  # float64 accumulation of < 2^14 rows, relative to the sum of absolute values


# ----------------------------------------------------------------------------- the keep mask
def hash3(a, b, c) -> np.ndarray:
    """The kernel's counter hash on uint32 arrays; every sum and product wraps modulo 2^32."""
    a, b, c = (np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in (a, b, c))
    M = np.uint64(0xFFFFFFFF)

    def mul(x, k):  # (x * k) mod 2^32: both factors are below 2^32, so the uint64 product is exact
        return (x * np.uint64(k)) & M

    h = mul(a, 0x9E3779B1) ^ mul((b + np.uint64(0x7F4A7C15)) & M, 0x85EBCA77) ^ \
        mul((c + np.uint64(0x165667B1)) & M, 0xC2B2AE3D)
    h = h ^ (h >> np.uint64(15))
    h = mul(h, 0x2C1B3C6D)
    h = h ^ (h >> np.uint64(12))
    h = mul(h, 0x297A2D39)
    h = h ^ (h >> np.uint64(15))
    return h.astype(np.uint32)


def mask_seed(seed: int, rank: int = 0) -> int:
    return (int(seed) + 0x9E3779B9 * int(rank)) & 0xFFFFFFFF


def keep_mask(seed: int, rnd: int, n: int, T: int, subsample: float) -> np.ndarray:
    """bool [n, T] of round ``rnd`` (absolute); ``seed`` is already masked / rank-mixed (:func:`mask_seed`)."""
    b = (int(rnd) * 131071 + np.arange(T, dtype=np.int64)) & 0xFFFFFFFF
    hsh = hash3(np.uint64(seed & 0xFFFFFFFF), b[None, :], np.arange(n, dtype=np.int64)[:, None])
    u = (hsh >> np.uint32(8)).astype(np.float64) * 2.0 ** -24  # < 2^24: exact in float32 as well
    return u < float(np.float32(subsample))


# ----------------------------------------------------------------------------- gradients and their bounds
def gradients(objective: str, m32: np.ndarray, Y: np.ndarray):
    """(g, h, dg, dh) float64 [n, T] from float32 margins and labels (one-hot for the multi-class objectives)."""
    assert m32.dtype == np.float32
    m = m32.astype(np.float64)
    y = np.asarray(Y, np.float32).astype(np.float64)
    T = m.shape[1]
    if objective in R.LOGISTIC:
        p = R._sigmoid64(m)
        b = np.full(m.shape, 2.0 ** -21)
        return p - y, np.maximum(p * (1.0 - p), 1e-16), b, b.copy()
    if objective == "reg:squarederror":
        g = m - y
        return g, np.ones_like(g), 2.0 ** -24 * np.abs(g), np.zeros_like(g)
    assert objective in R.MULTI
    p = R._softmax64(m)
    rel = (T + 4) * 2.0 ** -24
    return p - y, np.maximum(2.0 * p * (1.0 - p), 1e-16), rel * p + 2.0 ** -25, 2.0 * rel * p + 2.0 ** -24


# ----------------------------------------------------------------------------- budgets
def _term_budget(G, dG, H, dH, lam):
    """Largest change of G^2 / (H + lam) over G +- dG, H +- dH (inf where H - dH + lam <= 0)."""
    a = np.abs(G)
    lo_den, hi_den = H - dH + lam, H + dH + lam
    with np.errstate(divide="ignore", invalid="ignore"):
        t = a * a / (H + lam)
        up = (a + dG) ** 2 / lo_den
        dn = np.maximum(a - dG, 0.0) ** 2 / hi_den
        out = np.maximum(up - t, t - dn)
    return np.where(lo_den > 0, out, np.inf)


def _weight_budget(G, dG, H, dH, lam):
    """Largest change of G / (H + lam) over the same box (covers a sign change of G)."""
    a = abs(G)
    if H - dH + lam <= 0:
        return np.inf
    v = a / (H + lam)
    return max((a + dG) / (H - dH + lam) - v, v - max(a - dG, 0.0) / (H + dH + lam))


@dataclass
class NodeRec:
    """What the reference alone found at an open node (for the tests that build mutations)."""
    k: int
    node: int
    split: bool  # best gain > KRT_EPS
    f: int = -1
    b: int = 0
    gain: float = -np.inf
    bud: float = 0.0
    f2: int = -1  # the best other candidate
    b2: int = 0
    gain2: float = -np.inf
    bud2: float = 0.0
    followed: bool = False  # the regrow followed the engine here (ambiguous)


@dataclass
class Result:
    violations: list = field(default_factory=list)
    decisions: int = 0
    ambiguous: int = 0
    leaf: float = 0.0  # worst |dev - ref| / budget
    gain: float = 0.0
    cover: float = 0.0
    nodes: list = field(default_factory=list)
    min_open_h: float = np.inf  # smallest H - dH + lambda over the open nodes that hold rows (a precondition)
    max_abs_margin: float = 0.0  # largest |margin| any round started from

    def line(self, case: str) -> str:
        return (f"FIT-RATIO {case}: leaf {self.leaf:.4f} gain {self.gain:.4f} cover {self.cover:.4f} "
                f"ambiguous {self.ambiguous}/{self.decisions}")


def _ratio(diff: float, bud: float) -> float:
    if not np.isfinite(diff):
        return np.inf
    return diff / bud if bud > 0 else (0.0 if diff == 0 else np.inf)


class _Problem:
    def __init__(self, model, X, Y):
        self.cuts = model.cuts
        self.bins = R.bin_features(X, model.cuts)
        n, F = self.bins.shape
        self.n, self.F = n, F
        self.nbf = np.array([len(c) + 1 for c in model.cuts], dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.nbf)])
        self.C = int(self.off[-1])
        self.cell = self.bins + self.off[None, :-1]  # [n, F]
        self.cell_feat = np.repeat(np.arange(F), self.nbf)
        self.cell_bin = np.arange(self.C) - self.off[self.cell_feat]
        self.notlast = self.cell_bin < self.nbf[self.cell_feat] - 1
        assert (self.bins < self.nbf[None, :]).all()


def _left_sums(hist, P):
    """[no, C] cell sums -> sums over "bins <= b" within each feature's segment."""
    out = np.empty_like(hist)  # per segment, in bin order: two columns with the same bins get the same bits
    for f in range(P.F):
        np.cumsum(hist[:, P.off[f]:P.off[f + 1]], axis=1, out=out[:, P.off[f]:P.off[f + 1]])
    return out


def _grow(P, res, k, g, h, dg, dh, p, trees):
    """Regrow tree k from (g, h) with bounds (dg, dh), all [n]; returns the reference's arrays."""
    D, lam, mcw, gamma, eta = p["D"], p["lam"], p["mcw"], p["gamma"], p["eta"]
    NN = 2 ** (D + 1) - 1
    e_st, e_fe, e_sb = trees.status[k], trees.feat[k], trees.sbin[k]
    st = np.zeros(NN, np.int8)
    fe = np.full(NN, -1, np.int64)
    sb = np.zeros(NN, np.int64)
    gn, gb = np.zeros(NN), np.zeros(NN)
    Gs, Hs, dGs, dHs = (np.zeros(NN) for _ in range(4))
    ag, ah = np.abs(g), np.abs(h)
    st[0] = 2
    node = np.zeros(P.n, dtype=np.int64)
    Gs[0], Hs[0] = g.sum(), h.sum()
    dGs[0], dHs[0] = dg.sum() + SUM_SLACK * ag.sum(), dh.sum() + SUM_SLACK * ah.sum()
    bad = res.violations
    for depth in range(D):
        first, nl = 2 ** depth - 1, 2 ** depth
        open_nodes = [i for i in range(first, first + nl) if st[i] == 2]
        if not open_nodes:
            break
        slot = np.full(NN, -1, np.int64)
        slot[open_nodes] = np.arange(len(open_nodes))
        rs = slot[node]
        rows = np.nonzero(rs >= 0)[0]
        key = (rs[rows, None] * P.C + P.cell[rows]).ravel()
        size = len(open_nodes) * P.C

        def hist(w):
            return np.bincount(key, weights=np.repeat(w[rows], P.F), minlength=size).reshape(len(open_nodes), P.C)

        GL, HL = _left_sums(hist(g), P), _left_sums(hist(h), P)
        dGL = _left_sums(hist(dg), P) + SUM_SLACK * _left_sums(hist(ag), P)
        dHL = _left_sums(hist(dh), P) + SUM_SLACK * _left_sums(hist(ah), P)
        for j, i in enumerate(open_nodes):
            res.decisions += 1
            G, H, dG, dH = Gs[i], Hs[i], dGs[i], dHs[i]
            if (rs == j).any():
                res.min_open_h = min(res.min_open_h, H - dH + lam)
            gl, hl, dgl, dhl = GL[j], HL[j], dGL[j], dHL[j]
            gr, hr = G - gl, H - hl
            dgr, dhr = np.maximum(dG - dgl, 0.0), np.maximum(dH - dhl, 0.0)

            def ok(a, b):
                return P.notlast & (a >= mcw) & (b >= mcw) & (a + lam > 0) & (b + lam > 0)

            valid, sure, maybe = ok(hl, hr), ok(hl - dhl, hr - dhr), ok(hl + dhl, hr + dhr)
            with np.errstate(divide="ignore", invalid="ignore"):
                gain = gl * gl / (hl + lam) + gr * gr / (hr + lam) - G * G / (H + lam)
            bud = _term_budget(gl, dgl, hl, dhl, lam) + _term_budget(gr, dgr, hr, dhr, lam) + \
                _term_budget(G, dG, H, dH, lam)
            bud = np.where(np.isfinite(gain), bud, np.inf)
            sure = sure & np.isfinite(bud)
            vg = np.where(valid & np.isfinite(gain), gain, -np.inf)
            rec = NodeRec(k, i, False)
            cb = int(np.argmax(vg)) if P.C else 0
            best = vg[cb] if P.C else -np.inf
            if np.isfinite(best):
                rec.f, rec.b, rec.gain, rec.bud = int(P.cell_feat[cb]), int(P.cell_bin[cb]), float(best), float(bud[cb])
                v2 = vg.copy()
                v2[cb] = -np.inf
                c2 = int(np.argmax(v2))
                if np.isfinite(v2[c2]):
                    rec.f2, rec.b2, rec.gain2, rec.bud2 = (int(P.cell_feat[c2]), int(P.cell_bin[c2]), float(v2[c2]),
                                                           float(bud[c2]))
            nominal = bool(best > KRT_EPS)
            rec.split = nominal
            # what any engine inside the bounds must / may do
            with np.errstate(invalid="ignore"):
                lo = np.where(sure, gain - bud, -np.inf)
                hi = np.where(maybe, np.where(np.isfinite(gain), gain, np.inf) + bud, -np.inf)  # nan gain: unknown
            floor_ = float(lo.max()) if P.C else -np.inf
            must = floor_ > KRT_EPS
            may = bool((hi > KRT_EPS).any()) if P.C else False
            do_split, ce = nominal, cb
            if e_st[i] == 1:  # the engine shows its decision here
                f_e, b_e = int(e_fe[i]), int(e_sb[i])
                if not (0 <= f_e < P.F and 0 <= b_e < P.nbf[f_e] - 1):
                    bad.append((k, i, "split on a candidate that does not exist", f_e, b_e))
                else:
                    c_e = int(P.off[f_e] + b_e)
                    if nominal and c_e == cb:
                        pass
                    elif maybe[c_e] and hi[c_e] > KRT_EPS and hi[c_e] >= floor_:
                        res.ambiguous += 1
                        rec.followed = True
                    elif not may:
                        bad.append((k, i, "split where the best gain is below KRT_EPS", float(best), float(rec.bud)))
                    else:
                        bad.append((k, i, "split on another candidate than the best", (f_e, b_e, float(gain[c_e])),
                                    (rec.f, rec.b, rec.gain, rec.bud)))
                    do_split, ce = True, c_e  # follow the engine, so that one cause is reported once
            elif e_st[i] == 2 and must != may:  # within the budget of KRT_EPS: the engine's leaf is followed
                if nominal:
                    res.ambiguous += 1
                    rec.followed = True
                do_split = False
            res.nodes.append(rec)
            if not do_split:
                continue
            f, b = int(P.cell_feat[ce]), int(P.cell_bin[ce])
            st[i], fe[i], sb[i], gn[i], gb[i] = 1, f, b, gain[ce], bud[ce]
            l, r = 2 * i + 1, 2 * i + 2
            st[l] = st[r] = 2
            Gs[l], Hs[l], dGs[l], dHs[l] = gl[ce], hl[ce], dgl[ce], dhl[ce]
            Gs[r], Hs[r], dGs[r], dHs[r] = gr[ce], hr[ce], dgr[ce], dhr[ce]
            mine = node == i
            node[mine] = np.where(P.bins[mine, f] > b, r, l)
    # prune, bottom-up
    if gamma > 0:
        for i in range(2 ** D - 2, -1, -1):
            if st[i] != 1 or st[2 * i + 1] != 2 or st[2 * i + 2] != 2:
                continue
            prune = gn[i] < gamma
            if abs(gn[i] - gamma) <= gb[i] + STORE * gamma and e_st[i] in (1, 2):
                res.ambiguous += 1
                prune = e_st[i] == 2
            if prune:
                st[i], fe[i] = 2, -1
                st[2 * i + 1] = st[2 * i + 2] = 0
    return st, fe, sb, gn, gb, Gs, Hs, dGs, dHs


def _compare(res, k, ref, trees, p):
    st, fe, sb, gn, gb, Gs, Hs, dGs, dHs = ref
    lam, eta = p["lam"], p["eta"]
    bad = res.violations
    e_st, e_fe, e_sb = trees.status[k], trees.feat[k], trees.sbin[k]
    e_leaf, e_gain, e_cover = trees.leaf[k], trees.gain[k], trees.cover[k]
    for i in np.nonzero(e_st != st)[0]:
        bad.append((k, int(i), "status", int(e_st[i]), int(st[i])))
    for i in np.nonzero(e_fe != fe)[0]:
        bad.append((k, int(i), "feat", int(e_fe[i]), int(fe[i])))
    for i in range(len(st)):
        if st[i] == 0:
            if e_cover[i] != 0:
                bad.append((k, i, "cover of an unused node", float(e_cover[i]), 0.0))
            continue
        d = abs(float(e_cover[i]) - Hs[i])
        b = dHs[i] + STORE * abs(Hs[i])
        res.cover = max(res.cover, _ratio(d, b))
        if not d <= b:
            bad.append((k, i, "cover", float(e_cover[i]), float(Hs[i]), b))
        if st[i] == 1:
            if e_sb[i] != sb[i]:
                bad.append((k, i, "sbin", int(e_sb[i]), int(sb[i])))
            d = abs(float(e_gain[i]) - gn[i])
            b = gb[i] + STORE * abs(gn[i])
            res.gain = max(res.gain, _ratio(d, b))
            if not d <= b:
                bad.append((k, i, "gain", float(e_gain[i]), float(gn[i]), b))
        else:
            if Hs[i] + lam > 0:
                want = -Gs[i] / (Hs[i] + lam) * eta
                b = eta * _weight_budget(Gs[i], dGs[i], Hs[i], dHs[i], lam) + STORE * abs(want)
            else:
                want, b = 0.0, 0.0
            d = abs(float(e_leaf[i]) - want)
            res.leaf = max(res.leaf, _ratio(d, b))
            if not np.isfinite(e_leaf[i]):
                bad.append((k, i, "leaf is not finite", float(e_leaf[i])))
            elif not d <= b:
                bad.append((k, i, "leaf", float(e_leaf[i]), float(want), b))


def check_fit(model, X, Y, rank: int = 0, ties=()) -> Result:
    """Regrow and compare every tree of ``model`` (fitted on X, Y).  ``Y``: [n] or [n, T] targets, class ids for
    the multi-class objectives.  ``rank``: this process' rank when the fit was data-parallel (the keep mask's
    seed).  ``ties``: (lower, higher) pairs of columns with identical bins."""
    trees = model.trees
    T = int(model.n_tasks)
    objective = model.objective
    Y = np.asarray(Y, np.float64)
    if objective in R.MULTI:
        Y = np.eye(T)[Y.reshape(-1).astype(np.int64)]
    elif Y.ndim == 1:
        Y = Y[:, None]
    P = _Problem(model, X, Y)
    assert Y.shape == (P.n, T) and trees.status.shape[0] % T == 0
    assert P.n < 1 << 14, "SUM_SLACK covers fewer than 2^14 rows"
    p = dict(D=int(trees.max_depth), lam=float(model.lam), mcw=float(model.mcw), gamma=float(model.gamma),
             eta=float(model.eta))
    s = int(getattr(model, "quant_bits_used", 0))
    sub = float(model.subsample)
    seed = mask_seed(model.seed, rank)
    res = Result()
    m = np.full((P.n, T), np.float32(model.base_margin), dtype=np.float32)
    for rnd in range(trees.status.shape[0] // T):
        res.max_abs_margin = max(res.max_abs_margin, float(np.abs(m).max()))
        g, h, dg, dh = gradients(objective, m, Y)
        if s:
            dg, dh = dg + 2.0 ** -(s + 1), dh + 2.0 ** -s
        if sub < 1.0:
            keep = keep_mask(seed, rnd, P.n, T, sub).astype(np.float64)
            g, h, dg, dh = g * keep, h * keep, dg * keep, dh * keep
        for t in range(T):
            k = rnd * T + t
            ref = _grow(P, res, k, g[:, t], h[:, t], dg[:, t], dh[:, t], p, trees)
            _compare(res, k, ref, trees, p)
            m[:, t] = (m[:, t] + R.leaf_values(trees, P.bins, k)).astype(np.float32)
    for lo, hi_ in ties:
        assert np.array_equal(P.bins[:, lo], P.bins[:, hi_]) and lo < hi_
        for k, i in zip(*np.nonzero((trees.status == 1) & (trees.feat == hi_))):
            res.violations.append((int(k), int(i), "exact tie resolved to the higher feature", hi_, lo))
    return res
