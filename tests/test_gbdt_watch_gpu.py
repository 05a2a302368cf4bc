"""The GBDT watch-list metrics (K13 and its fused forms) and ``em_gbdt_predict`` (K11) against the fp64
reference of tests/_gbdt_ref.py: every round, every watch set and the train metric, for every metric and
objective on every driver path (fused round with the update inside the next level-0 histogram pass, separate
launches, more than four watch sets, chunked ``em_gbdt_fit`` calls, fixed-point histograms,
element counts past the 4096-block grid cap, the one-rank data-parallel path).

The reference is built from the fitted model's own trees and cuts, so a metric failure cannot hide behind a
tree difference; where the numpy oracle is cheap its tree structure is compared as well.  Budgets and their
preconditions: tests/_gbdt_ref.py (proved on the CPU by tests/test_gbdt_ref_cpu.py).  Each test prints the
worst |dev - ref| / budget it saw (``pytest -s``)."""
import functools

import numpy as np
import pytest

import _gbdt_ref as R
import _gbdt_watch_data as D
from euromillioner_amd.models import gbdt as G

pytestmark = pytest.mark.gpu

DRIVERS = ("default", "separate")
TREE_ARRAYS = ("status", "feat", "sbin", "leaf", "gain", "cover")
_models: dict = {}


@functools.lru_cache(maxsize=None)
def _sets(objective):
    return D.problem(objective)


@functools.lru_cache(maxsize=None)
def _large():
    return D.large_problem()


def _new(objective, metric, driver="default", **kw):
    g = G.GBDT(objective=objective, eval_metric=metric, backend="hip", **dict(D.KW, **kw))
    g.separate_launches = driver == "separate"
    return g


def _fit(objective, metric, n_sets=4, driver="default", **kw):
    """A HIP fit on the standard problem with the first ``n_sets`` watch sets (fitted once per configuration)."""
    key = (objective, metric, n_sets, driver, tuple(sorted(kw.items())))
    if key not in _models:
        sets = _sets(objective)
        m = _new(objective, metric, driver, **kw).fit(*sets["train"], evals=D.watch(sets, n_sets))
        assert m.backend_used == "hip" and m.eval_metric == metric
        _models[key] = m
    return _models[key]


@functools.lru_cache(maxsize=None)
def _oracle(objective, **kw):
    return G.GBDT(objective=objective, backend="numpy", **dict(D.KW, **dict(kw))).fit(*_sets(objective)["train"])


def _check(m, evals, train, path):
    """Every round of every set (and of the train metric, with ``train``) inside its budget."""
    refs = D.refs_for(R, m, evals, train=train)
    bad = R.compare_history(m.history, m.train_history if train is not None else None, refs)
    print(f"\nWATCH-RATIO {path}: worst |dev - ref| / budget = "
          f"{R.worst_ratio(m.history, m.train_history, refs):.4f} over {sum(len(v) for v in refs.values())} values")
    assert bad == [], bad
    if train is not None and "train" in evals:  # the watch set over the training rows: the same terms, regrouped
        assert len(m.train_history) == len(m.history)
        for rec, tv in zip(m.history, m.train_history):
            assert R.same_within(rec["train"], tv), (rec, tv)
    return refs


def _same_structure(m, objective, **kw):
    o = _oracle(objective, **kw)
    for k in ("status", "feat", "sbin"):
        assert np.array_equal(getattr(m.trees, k), getattr(o.trees, k)), k


# ----------------------------------------------------------------------------- matrix A
MATRIX_A = [(o, mt, d) for o, mt in D.PAIRS for d in (DRIVERS if not o.startswith("multi:") else DRIVERS[:1])]


@pytest.mark.parametrize("objective,metric,driver", MATRIX_A,
                         ids=[f"{o.split(':')[1]}-{mt}-{d}" for o, mt, d in MATRIX_A])
def test_watch_list_every_round_and_set(objective, metric, driver):
    sets = _sets(objective)
    m = _fit(objective, metric, 4, driver)
    assert m.trees.n_trees == 12 * m.n_tasks and (m.trees.status == 1).sum() > m.trees.n_trees
    _same_structure(m, objective)
    _check(m, D.watch(sets, 4), sets["train"], f"A {objective} {metric} {driver}")


def test_split_final_max_depth_is_8():
    """The deep case below must be the smallest depth past the fused round's limit."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "gbdt.hip")).read()
    assert re.search(r"constexpr int SPLIT_FINAL_MAX_DEPTH = (\d+);", src).group(1) == "8"


@pytest.mark.parametrize("depth", [1, 9])
def test_watch_list_shallow_and_past_the_fused_depth(depth):
    """Depth 1 (the root split finalises the tree) and depth 9 = SPLIT_FINAL_MAX_DEPTH + 1 (the non-fused
    driver with an elementwise metric)."""
    sets = _sets("reg:logistic")
    m = _fit("reg:logistic", "logloss", 4, max_depth=depth)
    _same_structure(m, "reg:logistic", max_depth=depth)
    _check(m, D.watch(sets, 4), sets["train"], f"A reg:logistic logloss depth {depth}")


@pytest.mark.parametrize("driver", ["default", "separate"])
def test_train_metric_without_watch_sets(driver):
    """No watch set at all: the per-round metric table is the train column alone."""
    sets = _sets("reg:logistic")
    m = _fit("reg:logistic", "logloss", 0, driver)
    assert m.history == [{"round": r} for r in range(12)] and len(m.train_history) == 12
    _check(m, {}, sets["train"], f"A no watch set {driver}")
    four = _fit("reg:logistic", "logloss", 4, driver)
    assert np.array_equal(m.trees.leaf, four.trees.leaf)
    assert all(R.same_within(a, b) for a, b in zip(m.train_history, four.train_history))


# ----------------------------------------------------------------------------- matrix B
@pytest.mark.parametrize("objective,metric", [D.PAIRS[0], D.PAIRS[1], D.PAIRS[2]],
                         ids=["logistic-logloss", "logistic-error", "squarederror-rmse"])
@pytest.mark.parametrize("n_sets", [5, 6])
def test_more_than_four_watch_sets(objective, metric, n_sets):
    """n_evals > 4: last-arriving-block metrics (live counter, one launch per set, one shared partial region)."""
    sets = _sets(objective)
    m = _fit(objective, metric, n_sets)
    _check(m, D.watch(sets, n_sets), sets["train"], f"B {objective} {metric} {n_sets} sets")
    four = _fit(objective, metric, 4)
    for k in TREE_ARRAYS:
        assert np.array_equal(getattr(m.trees, k), getattr(four.trees, k)), k
    for ra, rb in zip(m.history, four.history):
        for name in D.ORDER[:4]:
            assert R.same_within(ra[name], rb[name]), (name, ra, rb)
    for ta, tb in zip(m.train_history, four.train_history):
        assert R.same_within(ta, tb)


# ----------------------------------------------------------------------------- chunked calls
@pytest.mark.parametrize("driver", ["default", "separate"])
def test_chunked_fit_calls(driver, monkeypatch):
    """rounds_per_call = 3 over 7 rounds: em_gbdt_fit runs with r0 = 0, 3 and 6 (a one-round last chunk)."""
    from euromillioner_amd.models import gbdt_hip

    sets = _sets("reg:logistic")
    ev = D.watch(sets, 4)
    whole = _fit("reg:logistic", "logloss", 4, driver, nround=7)
    monkeypatch.setattr(gbdt_hip, "fit", functools.partial(gbdt_hip.fit, rounds_per_call=3))
    m = _new("reg:logistic", "logloss", driver, nround=7).fit(*sets["train"], evals=ev)
    for k in TREE_ARRAYS:
        assert np.array_equal(getattr(m.trees, k), getattr(whole.trees, k)), k
    assert len(m.history) == len(m.train_history) == 7
    for ra, rb in zip(m.history, whole.history):
        assert ra.keys() == rb.keys() and all(R.same_within(ra[k], rb[k]) for k in ra), (ra, rb)
    for ta, tb in zip(m.train_history, whole.train_history):
        assert R.same_within(ta, tb)
    _check(m, ev, sets["train"], f"chunked {driver}")
    _check(whole, ev, sets["train"], f"single call, 7 rounds, {driver}")


# ----------------------------------------------------------------------------- past the grid cap
LARGE_PAIRS = [("reg:logistic", "error"), ("reg:squarederror", "rmse")]


def _fit_large(objective, metric, case, driver="default"):
    key = ("large", objective, metric, case, driver)
    if key not in _models:
        s = _large()
        if case == "watch":  # a 17 000-row watch set on a 600-row fit
            train, ev, kw = s["small"], {"train": s["small"], "large": s["large"], "b": s["b"]}, dict(nround=4)
        elif case == "watch5":  # the same with five sets: gbdt_predict_metric's own launches
            lx, ly = s["large"]
            train, kw = s["small"], dict(nround=4)
            ev = {"train": s["small"], "large": s["large"], "b": s["b"], "la": (lx[:255], ly[:255]),
                  "one": (lx[-1:], ly[-1:])}
        else:  # the 17 000 rows as the training set
            train, ev, kw = s["large"], {"train": s["large"], "b": s["b"]}, dict(nround=3)
        m = _new(objective, metric, driver, **kw).fit(*train, evals=ev)
        assert m.backend_used == "hip" and m.n_tasks == 62
        _models[key] = (m, ev, train)
    return _models[key]


@pytest.mark.parametrize("objective,metric", LARGE_PAIRS, ids=["logistic-error", "squarederror-rmse"])
@pytest.mark.parametrize("case,driver", [("watch", "default"), ("watch", "separate"), ("watch5", "default"),
                                         ("train", "default"), ("train", "separate")])
def test_past_the_grid_cap(objective, metric, case, driver):
    """62 x 17 000 elements > 4096 blocks x 256 threads: the grid-stride loops take a second trip; exact error
    counts and rmse show a single element missed on it."""
    m, ev, train = _fit_large(objective, metric, case, driver)
    assert 62 * D.N_LARGE > 4096 * 256 and len(ev["large" if case != "train" else "train"][0]) == D.N_LARGE
    _check(m, ev, train, f"grid cap {objective} {metric} {case} {driver}")


# ----------------------------------------------------------------------------- quantised histograms
@pytest.mark.parametrize("metric", ["logloss", "error"])
def test_watch_list_quantised_histograms(metric):
    """hist_mode="quant": the separate-launch driver with deferred metrics."""
    sets = _sets("reg:logistic")
    m = _fit("reg:logistic", metric, 4, hist_mode="quant")
    assert m.quant_bits_used > 0
    _same_structure(m, "reg:logistic", hist_mode="quant")
    _check(m, D.watch(sets, 4), sets["train"], f"quant {metric}")


# ----------------------------------------------------------------------------- one-rank process group
def test_one_rank_group_error_counts():
    """The data-parallel path's metric (em_gbdt_predict + em_gbdt_metric_sum per round and set): exact error
    counts in every round; it keeps no train metric."""
    import socket

    import torch
    import torch.distributed as dist

    sets = _sets("reg:logistic")
    ev = D.watch(sets, 4)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        m = _new("reg:logistic", "error").fit(*sets["train"], evals=ev, group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
    assert m.train_history == []
    refs = _check(m, ev, None, "one-rank group error")
    assert all(ref.errors is not None for rr in refs.values() for ref in rr)
    single = _fit("reg:logistic", "error", 4)
    for k in ("status", "feat", "sbin", "leaf"):
        assert np.array_equal(getattr(m.trees, k), getattr(single.trees, k)), k


# ----------------------------------------------------------------------------- em_gbdt_predict
def _predict_direct(m, X, k0, k1, m0):
    """em_gbdt_predict on trees [k0, k1) over a margin buffer pre-filled with m0 [n, T]; returns [n, T]."""
    import torch

    from euromillioner_amd.models import gbdt_hip  # noqa: F401  (registers the signatures)
    from euromillioner_amd.ops import _native as N

    dev = torch.device("cuda", torch.cuda.current_device())
    status, feat, sbin, leaf = m._device_trees
    bins = G.apply_bins(np.asarray(X, np.float64), m.cuts)
    n, F = bins.shape
    T = m.n_tasks
    assert 0 <= k0 <= k1 <= m.trees.n_trees and status.numel() == m.trees.status.size and F == len(m.cuts)
    d_bins = torch.from_numpy(np.ascontiguousarray(bins, dtype=np.uint8)).to(dev)
    margin = torch.from_numpy(np.ascontiguousarray(m0.T, dtype=np.float32).reshape(-1)).to(dev)
    N.call("em_gbdt_predict", d_bins.data_ptr(), margin.data_ptr(), T, n, F, m.trees.max_depth, k0, k1,
           status.data_ptr(), feat.data_ptr(), sbin.data_ptr(), leaf.data_ptr(), N.stream_handle(dev))
    torch.cuda.synchronize()
    return margin.view(T, n).t().cpu().numpy()


def _pattern(n, T):
    r, t = np.meshgrid(np.arange(n), np.arange(T), indexing="ij")
    return (0.25 + 0.001 * ((7 * t + 3 * r) % 97) - 0.03 * t).astype(np.float32)


def _check_predict(m, X, k0, k1, path):
    T = m.n_tasks
    m0 = _pattern(len(X), T)
    got = _predict_direct(m, X, k0, k1, m0)
    s, a, cnt = R.predict_range(m.trees, m.cuts, T, X, k0, k1)
    want = m0.astype(np.float64) + s
    bud = cnt[None, :] * 2.0 ** -24 * (np.abs(m0).astype(np.float64) + a)  # cnt float32 additions per element
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bud).all(), (path, float(err.max()), np.argwhere(err > bud)[:5])
    untouched = cnt == 0  # tasks without a tree in the range: bit-identical
    assert np.array_equal(got[:, untouched].view(np.uint32), m0[:, untouched].view(np.uint32))
    live = bud > 0
    return float((err[live] / bud[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("k0,k1", [(0, 60), (5, 10), (7, 23), (59, 60), (13, 13)])
def test_predict_tree_ranges(k0, k1):
    """Tree ranges that start and end inside a round (k0 % T != 0), a single tree, the empty range; the
    kernel accumulates into the buffer."""
    sets = _sets("reg:logistic")
    m = _fit("reg:logistic", "logloss", 4)
    assert m.trees.n_trees == 60 and m.n_tasks == 5
    worst = 0.0
    for name in ("one", "a", "b"):
        assert len(sets[name][0]) in (1, 255, 257)
        worst = max(worst, _check_predict(m, sets[name][0], k0, k1, (name, k0, k1)))
    print(f"\nWATCH-RATIO predict [{k0}, {k1}): worst |dev - ref| / budget = {worst:.4f}")
    if k0 == k1:
        m0 = _pattern(257, 5)
        assert np.array_equal(_predict_direct(m, sets["b"][0], k0, k1, m0).view(np.uint32), m0.view(np.uint32))


def test_predict_tree_range_past_the_grid_cap():
    m, ev, train = _fit_large("reg:squarederror", "rmse", "watch")
    assert m.trees.n_trees >= 62
    worst = _check_predict(m, ev["large"][0], 3, 58, "large")
    print(f"\nWATCH-RATIO predict [3, 58) x 62 tasks x 17000 rows: worst |dev - ref| / budget = {worst:.4f}")


def test_predict_matches_reference_margins():
    """GBDT.predict_margin (trees 0 .. K over a base-margin buffer) against the replayed float32 margins."""
    sets = _sets("reg:logistic")
    m = _fit("reg:logistic", "logloss", 4)
    for name in ("one", "b"):
        X = sets[name][0]
        s, a, cnt = R.predict_range(m.trees, m.cuts, 5, X, 0, 60)
        got = m.predict_margin(X, backend="hip")
        assert (np.abs(got - (m.base_margin + s)) <= cnt[None, :] * 2.0 ** -24 * (abs(m.base_margin) + a)).all()


# ----------------------------------------------------------------------------- all-pruned trees
def test_all_pruned_trees():
    """gamma so large that every tree is a root leaf: metrics and predict stay inside their budgets."""
    sets = _sets("reg:logistic")
    m = _fit("reg:logistic", "logloss", 4, gamma=1e6)
    assert (m.trees.status[:, 0] == 2).all() and (m.trees.status[:, 1:] == 0).all()
    assert (m.trees.leaf[:, 0] != 0).any()
    _check(m, D.watch(sets, 4), sets["train"], "all-pruned")
    worst = max(_check_predict(m, sets[name][0], 0, 60, name) for name in ("one", "a", "b"))
    print(f"\nWATCH-RATIO predict all-pruned: worst |dev - ref| / budget = {worst:.4f}")
