"""tests/_gbdt_fit_ref.py proved without a GPU: a hand-computed tree, the numpy engine's trees of every case of
tests/test_gbdt_fit_gpu.py (no violations, inside the ambiguity cap), mutations of passing models and inputs that
the reference must reject, the uint32 hash mirror, and the ``reg_lambda = 0, min_child_weight = 0`` rule."""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import _gbdt_fit_cases as K
import _gbdt_fit_ref as FR
import _gbdt_watch_data as D
from euromillioner_amd.models import gbdt as G


@functools.lru_cache(maxsize=None)
def _fit(case, **over):
    dn, objective, kw = K.CASES[case]
    X, Y, _ = K.data(dn)
    return G.GBDT(objective=objective, backend="numpy", **dict(kw, **dict(over))).fit(X, Y)


def _run(m, case, Y=None):
    X, Y0, ties = K.data(K.CASES[case][0])
    return FR.check_fit(m, X, Y0 if Y is None else Y, ties=ties)


def _clone(m):
    """A copy whose tree arrays can be mutated (the fitted models are shared between the tests)."""
    c = copy.copy(m)
    c.trees = copy.copy(m.trees)
    for k in ("status", "feat", "sbin", "leaf", "gain", "cover"):
        setattr(c.trees, k, getattr(m.trees, k).copy())
    return c


# ----------------------------------------------------------------------------- hand example
def _hand_model():
    """8 rows, 2 binary features, squared error from margin 0 (g = -y, h = 1), lambda = 1, eta = 1, mcw = 1.

    rows (f0, f1, y): (0,0,0) (0,0,0) (0,1,0) (0,1,1) | (1,0,2) (1,0,2) (1,1,10) (1,1,10)

    root: G = -25, H = 8, G^2/(H+1) = 625/9.
      f0: left G = -1, H = 4 -> 1/5; right G = -24, H = 4 -> 576/5; gain = 115.4 - 625/9 = 45.9555...
      f1: left G = -4, H = 4 -> 16/5; right G = -21, H = 4 -> 441/5; gain = 91.4 - 625/9 = 21.9555...  -> f0 wins
    node 1 (f0 = 0): G = -1, H = 4, term 1/5.  f1: left G = 0, H = 2 -> 0; right G = -1, H = 2 -> 1/3;
      gain = 1/3 - 1/5 = 0.1333...; f0: the right side is empty (H = 0 < mcw), no candidate.
    node 2 (f0 = 1): G = -24, H = 4, term 576/5.  f1: left G = -4, H = 2 -> 16/3; right G = -20, H = 2 -> 400/3;
      gain = 416/3 - 576/5 = 23.4666...
    gamma = 1 lies between 0.1333 and 23.4666: node 1's split is pruned (leaf 1/5), node 2's stays (leaves
    4/3 and 20/3); the root stays, its children are not both leaves."""
    X = np.array([[0, 0], [0, 0], [0, 1], [0, 1], [1, 0], [1, 0], [1, 1], [1, 1]], dtype=np.float64)
    y = np.array([0, 0, 0, 1, 2, 2, 10, 10], dtype=np.float64)
    NN = 7
    tr = SimpleNamespace(max_depth=2, status=np.zeros((1, NN), np.int8), feat=np.full((1, NN), -1, np.int32),
                         sbin=np.zeros((1, NN), np.int32), leaf=np.zeros((1, NN)), gain=np.zeros((1, NN)),
                         cover=np.zeros((1, NN)))
    tr.status[0, [0, 2]] = 1
    tr.status[0, [1, 5, 6]] = 2
    tr.feat[0, 0], tr.feat[0, 2] = 0, 1
    tr.gain[0, 0], tr.gain[0, 2] = 115.4 - 625 / 9, 416 / 3 - 576 / 5
    tr.leaf[0, 1], tr.leaf[0, 5], tr.leaf[0, 6] = 1 / 5, 4 / 3, 20 / 3
    tr.cover[0, [0, 1, 2, 5, 6]] = [8, 4, 4, 2, 2]
    m = SimpleNamespace(trees=tr, cuts=[np.array([0.5]), np.array([0.5])], n_tasks=1, objective="reg:squarederror",
                        lam=1.0, mcw=1.0, gamma=1.0, eta=1.0, subsample=1.0, seed=0, base_margin=0.0,
                        quant_bits_used=0)
    return m, X, y


def test_hand_computed_two_level_tree():
    m, X, y = _hand_model()
    res = FR.check_fit(m, X, y)
    assert res.violations == [] and res.ambiguous == 0 and res.decisions == 3
    recs = {r.node: r for r in res.nodes}
    assert (recs[0].f, recs[0].b, recs[0].f2) == (0, 0, 1)
    assert abs(recs[0].gain - 45.955555555555556) < 1e-12 and abs(recs[0].gain2 - 21.955555555555556) < 1e-12
    assert recs[1].split and abs(recs[1].gain - 0.13333333333333333) < 1e-12  # split, then pruned by gamma = 1
    assert abs(recs[2].gain - 23.466666666666667) < 1e-12
    # the numpy engine grows the same tree
    o = G.GBDT(objective="reg:squarederror", base_score=0.0, nround=1, max_depth=2, gamma=1.0, eta=1.0,
               backend="numpy").fit(X, y)
    assert np.array_equal(o.trees.status, m.trees.status) and np.array_equal(o.trees.feat, m.trees.feat)
    assert np.allclose(o.trees.leaf, m.trees.leaf, rtol=1e-6) and np.array_equal(o.trees.cover, m.trees.cover)
    assert FR.check_fit(o, X, y).violations == []
    # and the hand tree with node 1's split kept is rejected
    m.trees.status[0, 1], m.trees.status[0, [3, 4]] = 1, 2
    m.trees.feat[0, 1], m.trees.gain[0, 1] = 1, 1 / 3 - 1 / 5
    m.trees.leaf[0, 1], m.trees.leaf[0, 4], m.trees.cover[0, [3, 4]] = 0.0, 1 / 3, 2
    assert any(v[2] == "status" for v in FR.check_fit(m, X, y).violations)


# ----------------------------------------------------------------------------- the numpy engine's trees
EXACT = {"std-logistic": 356, "std-squarederror": 412, "std-softprob": 266, "quant-std-logistic": 356,
         "par-ref": 342}  # decisions of the five named configurations; none of them ambiguous


@pytest.mark.parametrize("case", list(K.CASES))
def test_numpy_engine_passes_every_gpu_case(case):
    """No violations and the ambiguous count inside the cap of the GPU tests: the cap is met by the inputs."""
    m = _fit(case)
    res = _run(m, case)
    print("\n" + res.line(case + " (numpy)"))
    assert res.violations == [], res.violations[:10]
    assert res.ambiguous <= K.cap(res), (res.ambiguous, res.decisions)
    if case in EXACT:
        assert (res.ambiguous, res.decisions) == (0, EXACT[case])
        assert max(res.leaf, res.gain, res.cover) < 0.5
    if case == "par-zero":
        assert res.max_abs_margin <= 8.0 and res.min_open_h > 0
    if case.startswith("quant-"):
        assert m.quant_bits_used > 40
    if case == "dropped-all":
        assert (m.trees.status[:, 0] == 2).all() and (m.trees.leaf == 0).all()


def test_partial_pruning_gamma_case():
    base = _fit("std-logistic")
    gamma = K.partial_gamma(base.trees.gain[base.trees.status == 1])
    m = _fit("std-logistic", gamma=gamma)
    res = _run(m, "std-logistic")
    assert res.violations == [] and res.ambiguous <= K.cap(res)
    st = m.trees.status
    pruned = [r for r in res.nodes if r.split and st[r.k, r.node] == 2]
    assert pruned and 0 < (st == 1).sum() < (base.trees.status == 1).sum()
    assert any(r.node > 0 and st[r.k, (r.node - 1) // 2] == 1 for r in pruned)


def test_edge_columns_case():
    m = _fit("edge")
    (lo, hi), = K.data("edge")[2]
    feats = m.trees.feat[m.trees.status == 1]
    assert (feats == lo).any() and not (feats == hi).any() and not np.isin(feats, K.EDGE_CONST).any()


# ----------------------------------------------------------------------------- mutations
def _rejected(m, case, what=None, Y=None):
    res = _run(m, case, Y)
    assert res.violations, "the mutation passed"
    if what is not None:
        assert any(what in v[2] for v in res.violations), res.violations[:5]
    return res


def _clear_gap(r):
    return r.split and r.f2 >= 0 and r.gain2 > 1e-3 and r.gain - r.gain2 > 4 * (r.bud + r.bud2)


def test_mutation_second_best_split():
    m = _clone(_fit("std-logistic"))
    r = next(r for r in _run(m, "std-logistic").nodes if _clear_gap(r) and m.trees.status[r.k, r.node] == 1)
    m.trees.feat[r.k, r.node], m.trees.sbin[r.k, r.node] = r.f2, r.b2
    _rejected(m, "std-logistic", "another candidate")


def test_mutation_sbin_off_by_one():
    m = _clone(_fit("int8"))
    nb = [len(c) + 1 for c in m.cuts]
    r = next(r for r in _run(m, "int8").nodes
             if _clear_gap(r) and m.trees.status[r.k, r.node] == 1 and r.b + 1 < nb[r.f] - 1)
    m.trees.sbin[r.k, r.node] += 1
    _rejected(m, "int8", "another candidate")
    m = _clone(_fit("std-logistic"))  # on a one-hot feature bin 1 is the last bin: no candidate at all
    k, i = np.argwhere(m.trees.status == 1)[5]
    m.trees.sbin[k, i] += 1
    _rejected(m, "std-logistic", "does not exist")


def test_mutation_leaf_scaled():
    m = _clone(_fit("std-logistic"))
    k, i = np.argwhere((m.trees.status == 2) & (np.abs(m.trees.leaf) > 0.05))[7]
    m.trees.leaf[k, i] *= 1 + 1e-4
    res = _rejected(m, "std-logistic", "leaf")
    assert res.violations[0][:3] == (k, i, "leaf")  # the tree itself is reported, before its effect on later rounds


def test_mutation_cover():
    base = _fit("std-logistic")
    k, i = np.argwhere(base.trees.status == 2)[9]
    m = _clone(base)
    m.trees.cover[k, i] = 0.0
    (v,) = _rejected(m, "std-logistic", "cover").violations  # nothing else depends on a cover
    assert v[:4] == (k, i, "cover", 0.0) and abs(v[4] - base.trees.cover[k, i]) <= 1e-6 * v[4] and v[5] < 1e-3
    m = _clone(base)
    m.trees.cover[k, i] = m.trees.cover[k, (i - 1) // 2]
    assert len(_rejected(m, "std-logistic", "cover").violations) == 1


def test_mutation_gain_of_the_child():
    m = _clone(_fit("std-logistic"))
    st = m.trees.status
    k, i = next((k, i) for k, i in np.argwhere(st == 1) if 2 * i + 1 < st.shape[1] and st[k, 2 * i + 1] == 1)
    m.trees.gain[k, i] = m.trees.gain[k, 2 * i + 1]
    assert [v[:3] for v in _rejected(m, "std-logistic", "gain").violations] == [(k, i, "gain")]


def test_mutation_pruning_flipped():
    base = _fit("par-ref")  # gamma = 1
    res = _run(base, "par-ref")
    st = base.trees.status
    band = lambda r: r.bud + FR.STORE * base.gamma  # noqa: E731
    # a split the engine pruned, well below gamma: put it back
    r = next(r for r in res.nodes if r.split and st[r.k, r.node] == 2 and r.gain < base.gamma - 10 * band(r))
    m = _clone(base)
    m.trees.status[r.k, r.node], m.trees.status[r.k, [2 * r.node + 1, 2 * r.node + 2]] = 1, 2
    m.trees.feat[r.k, r.node], m.trees.sbin[r.k, r.node], m.trees.gain[r.k, r.node] = r.f, r.b, r.gain
    _rejected(m, "par-ref", "status")
    # a split that stayed, well above gamma, with two leaves below it: prune it
    r = next(r for r in res.nodes if st[r.k, r.node] == 1 and st[r.k, 2 * r.node + 1] == 2
             and st[r.k, 2 * r.node + 2] == 2 and r.gain > base.gamma + 10 * band(r))
    m = _clone(base)
    m.trees.status[r.k, r.node], m.trees.status[r.k, [2 * r.node + 1, 2 * r.node + 2]] = 2, 0
    m.trees.feat[r.k, r.node] = -1
    _rejected(m, "par-ref", "status")


def test_mutation_split_below_krt_eps():
    base = _fit("std-logistic")
    res = _run(base, "std-logistic")
    D_ = base.trees.max_depth
    r = next(r for r in res.nodes if not r.split and base.trees.status[r.k, r.node] == 2
             and r.node < 2 ** D_ - 1 and (r.f < 0 or r.gain + r.bud < FR.KRT_EPS))
    m = _clone(base)
    m.trees.status[r.k, r.node], m.trees.status[r.k, [2 * r.node + 1, 2 * r.node + 2]] = 1, 2
    m.trees.feat[r.k, r.node], m.trees.sbin[r.k, r.node], m.trees.gain[r.k, r.node] = max(r.f, 0), 0, 1e-3
    _rejected(m, "std-logistic", "below KRT_EPS")


def test_mutation_label_flipped_after_the_fit():
    X, Y, _ = K.data("std")
    Y = Y.copy()
    Y[123, 2] = 1.0 - Y[123, 2]
    res = _rejected(_fit("std-logistic"), "std-logistic", Y=Y)
    assert res.violations[0][0] == 2  # round 0's tree of task 2 already


def _fit_with_mask(monkeypatch, mask):
    monkeypatch.setattr(G, "subsample_keep", mask)
    dn, objective, kw = K.CASES["sub-0.5-logistic"]
    X, Y, _ = K.data(dn)
    return G.GBDT(objective=objective, backend="numpy", **kw).fit(X, Y)


def test_mutation_keep_mask_of_round_0(monkeypatch):
    keep = G.subsample_keep
    m = _fit_with_mask(monkeypatch, lambda seed, rnd, n, T, s: keep(seed, 0, n, T, s))
    res = _rejected(m, "sub-0.5-logistic")
    assert min(v[0] for v in res.violations) // m.n_tasks == 1  # round 0 passes, round 1 does not


def test_mutation_keep_mask_without_the_task(monkeypatch):
    keep = G.subsample_keep
    m = _fit_with_mask(monkeypatch, lambda seed, rnd, n, T, s: np.repeat(keep(seed, rnd, n, 1, s), T, axis=1))
    res = _rejected(m, "sub-0.5-logistic")
    assert min(v[0] for v in res.violations) == 1  # task 0 of round 0 passes, task 1 does not


def test_mutation_tie_to_the_higher_index():
    m = _clone(_fit("edge"))
    (lo, hi), = K.data("edge")[2]
    k, i = np.argwhere((m.trees.status == 1) & (m.trees.feat == lo))[0]
    m.trees.feat[k, i] = hi
    _rejected(m, "edge", "exact tie")


# ----------------------------------------------------------------------------- hash mirror
HAND = [((0, 0, 0), 0x84A50D3A),  # evaluated by hand with unbounded integers, reduced modulo 2^32 at every step
        ((12345, 11 * 131071 + 4, 649), 0x43384BA4),
        ((0xFFFFFFFF, (40000 * 131071 + 61) & 0xFFFFFFFF, 0x80000001), 0xDB4B0951)]


def test_hash_wraps_like_uint32():
    assert 40000 * 131071 + 61 > 1 << 32  # the round counter itself wraps in the third value
    for args, want in HAND:
        assert int(FR.hash3(*args)) == want
        assert int(G._hash3(*args)) == want  # the product's own copy
    big = FR.hash3(7, np.arange(5), np.arange(3)[:, None])
    assert big.shape == (3, 5) and big.dtype == np.uint32


def test_keep_rate_and_independence():
    n, T, s = 20000, 5, 0.3
    k = FR.keep_mask(99, 4, n, T, s)
    assert abs(k.mean() - s) < 5 * np.sqrt(s * (1 - s) / (n * T))  # 10^5 elements
    assert not np.array_equal(k, FR.keep_mask(99, 5, n, T, s))  # rounds
    assert not np.array_equal(k[:, 0], k[:, 1])  # tasks
    assert not np.array_equal(k, FR.keep_mask(100, 4, n, T, s))  # seeds
    for other in (FR.keep_mask(99, 5, n, T, s), k[:, [1, 2, 3, 4, 0]], FR.keep_mask(100, 4, n, T, s)):
        assert abs((k & other).mean() - s * s) < 5 * np.sqrt(s * s / (n * T))  # and independent of one another
    assert FR.keep_mask(1, 0, 100, 3, 1e-9).sum() == 0


def test_both_mirrors_draw_the_same_mask():
    """The product's uint32 arithmetic and the reference's uint64 arithmetic, the rank-mixed seed included."""
    for seed, rank, rnd in ((0, 0, 0), (12345, 0, 11), (2 ** 40 + 17, 3, 40000), (-5, 1, 2)):
        assert FR.mask_seed(seed, rank) == G.subsample_seed(seed, rank)
        a = FR.keep_mask(FR.mask_seed(seed, rank), rnd, 700, 62, 0.8)
        assert np.array_equal(a, G.subsample_keep(G.subsample_seed(seed, rank), rnd, 700, 62, 0.8))
    assert FR.mask_seed(1, 2) == (1 + 2 * 0x9E3779B9) & 0xFFFFFFFF


# ----------------------------------------------------------------------------- lambda = 0, min_child_weight = 0
def test_lambda_0_mcw_0_grows_past_empty_sides():
    """The numpy engine closed every node that had an empty side among its candidates (0 * 0 / (0 + 0) = NaN won
    the arg-max, and the isfinite test then closed the node): 20 splits, the roots, where a lambda or a
    min_child_weight of 1e-12 gave 278.  Such a candidate is not valid (XGBoost's CalcGain gives the side 0)."""
    X, Y = D.problem("reg:logistic")["train"]
    kw = dict(objective="reg:logistic", backend="numpy", nround=4, max_depth=4, eta=0.5, gamma=0.0)
    zero = G.GBDT(reg_lambda=0.0, min_child_weight=0.0, **kw).fit(X, Y)
    lam = G.GBDT(reg_lambda=1e-12, min_child_weight=0.0, **kw).fit(X, Y)
    mcw = G.GBDT(reg_lambda=0.0, min_child_weight=1e-12, **kw).fit(X, Y)
    n0, n1, n2 = ((m.trees.status == 1).sum() for m in (zero, lam, mcw))
    assert n0 > 200 and (zero.trees.status[:, 0] == 1).all() and (zero.trees.status[:, 1:3] == 1).any()
    assert abs(n0 - n1) <= 0.05 * n1 and abs(n0 - n2) <= 0.05 * n2  # (equal but for near-ties of tiny nodes)
    assert np.isfinite(zero.trees.leaf).all() and np.isfinite(zero.trees.gain).all()
    # _best_split_hist: an empty right side at lambda = 0 is no candidate, the real split is found
    hg = np.array([[1.0, -1.0, 0.0]])
    hh = np.array([[0.5, 0.5, 0.0]])
    gain, f, b, GL, HL = G._best_split_hist(hg, hh, 0.0, 1.0, 0.0, 0.0)
    assert (f, b) == (0, 0) and abs(gain - 4.0) < 1e-12


def test_leaf_of_a_node_without_hessian_is_zero():
    tr = G.TreeArrays(1, 1)
    tr.status[0, 0] = 2
    G._prune_and_leaves(tr, 0, np.zeros(3), np.zeros(3), 0.0, 0.0, 1.0, 1)
    assert tr.leaf[0, 0] == 0.0
