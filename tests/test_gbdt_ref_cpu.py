"""CPU self-checks of tests/_gbdt_ref.py, at the shapes tests/test_gbdt_watch_gpu.py runs on the device.

The helper's recomputed watch-list history (fp64 metrics of margins replayed from the fitted trees) must agree
with the numpy oracle's history in every round and set, inside the budgets the device is held to; the budgets'
preconditions hold on these data; and ``compare_history`` rejects a history shifted by a round, two sets'
columns swapped, a metric that lost its last row, and a metric with the tasks reversed."""
import copy
import functools

import numpy as np
import pytest

import _gbdt_ref as R
import _gbdt_watch_data as D
from euromillioner_amd.models import gbdt as G

PAIR_IDS = [f"{o.split(':')[1]}-{m}" for o, m in D.PAIRS]


@functools.lru_cache(maxsize=None)
def _fit(objective, metric):
    """(oracle model, its evals, the refs of every set and of the train metric, the per-set margins)."""
    sets = D.problem(objective)
    ev = D.watch(sets, 6)
    m = G.GBDT(objective=objective, eval_metric=metric, backend="numpy", **D.KW).fit(*sets["train"], evals=ev)
    assert m.eval_metric == metric
    margins = {k: R.margins_by_round(m.trees, m.cuts, m.n_tasks, m.base_margin, ex) for k, (ex, _) in ev.items()}
    refs = {k: R.reference(objective, metric, ev[k][1], margins[k]) for k in ev}
    refs[R.TRAIN] = refs["train"]
    return m, ev, refs, margins


@functools.lru_cache(maxsize=None)
def _fit_large(objective, metric):
    sets = D.large_problem()
    ev = {"large": sets["large"]}
    m = G.GBDT(objective=objective, eval_metric=metric, backend="numpy", **dict(D.KW, nround=3)).fit(
        *sets["small"], evals=ev)
    margins = {"large": R.margins_by_round(m.trees, m.cuts, m.n_tasks, m.base_margin, ev["large"][0])}
    refs = {"large": R.reference(objective, metric, ev["large"][1], margins["large"])}
    return m, ev, refs, margins


def _sets_of(bad):
    return {b[1] for b in bad}


@pytest.mark.parametrize("objective,metric", D.PAIRS, ids=PAIR_IDS)
def test_reference_agrees_with_oracle_every_round_and_set(objective, metric):
    m, ev, refs, margins = _fit(objective, metric)
    assert len(m.history) == D.KW["nround"] == len(m.train_history)
    assert [len(ev[k][0]) for k in D.ORDER] == [D.N_TRAIN, 1, 255, 257, 700, 103]
    assert (m.trees.status == 1).sum() > m.trees.n_trees  # real trees, not root leaves
    assert R.compare_history(m.history, m.train_history, refs) == []
    # the replayed margins are the oracle's own: its predictions are their float32 transform
    got = m.predict(ev["b"][0])
    want = G.transform(objective, margins["b"][-1]).astype(np.float32)
    assert np.allclose(got, want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("objective,metric", D.PAIRS, ids=PAIR_IDS)
def test_preconditions_hold(objective, metric):
    """R.reference asserts them per round (it raised in _fit otherwise); spelled out once more here."""
    m, ev, refs, margins = _fit(objective, metric)
    for k, mm in margins.items():
        for m32 in mm:
            assert R.count_of(metric, m32) < 1 << 22
            assert R.ambiguous(objective, metric, m32) == 0
            if metric == "logloss":
                assert np.abs(m32).max() <= 8.0
            if metric == "mlogloss":
                p = R._softmax64(m32.astype(np.float64))
                assert p[np.arange(len(p)), R._labels(ev[k][1], len(p))].min() > 1e-6


def test_preconditions_reject_bad_inputs():
    y = np.array([[1.0], [0.0]])
    with pytest.raises(AssertionError):
        R.check_preconditions("reg:logistic", "logloss", y, np.array([[0.5], [8.5]], np.float32))
    with pytest.raises(AssertionError):
        R.check_preconditions("reg:logistic", "error", y, np.array([[0.5], [2.0 ** -21]], np.float32))
    R.check_preconditions("reg:logistic", "error", y, np.array([[0.5], [0.0]], np.float32))  # p == 1/2: not above
    R.check_preconditions("reg:squarederror", "error", y, np.array([[0.5], [0.5]], np.float32))
    with pytest.raises(AssertionError):
        R.check_preconditions("multi:softprob", "merror", np.array([0, 1]),
                              np.array([[1.0, 1.0 + 2.0 ** -22], [0.0, 1.0]], np.float32))
    with pytest.raises(AssertionError):
        R.check_preconditions("multi:softprob", "mlogloss", np.array([0, 1]),
                              np.array([[0.0, 15.0], [0.0, 1.0]], np.float32))


def test_metric_definitions_by_hand():
    y = np.array([[1.0, 0.0], [0.0, 1.0]])
    m = np.array([[2.0, -1.0], [0.0, 0.25]], np.float32)
    p = 1 / (1 + np.exp(-m.astype(np.float64)))
    assert abs(R.metric("reg:logistic", "logloss", y, m) + np.mean(y * np.log(p) + (1 - y) * np.log(1 - p))) < 1e-15
    assert R.error_count("reg:logistic", "error", y, m) == 0  # m == 0 -> p == 0.5 -> class 0
    assert R.error_count("reg:squarederror", "error", y, m) == 1  # 0.25 is not above 0.5
    assert abs(R.metric("reg:squarederror", "rmse", y, m) - np.sqrt((1 + 1 + 0 + 0.5625) / 4)) < 1e-15
    mc = np.array([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0]], np.float32)
    assert R.error_count("multi:softprob", "merror", np.array([1, 1]), mc) == 1  # first maximum: classes 0, 1
    e = np.exp([1.0, 1.0, 0.0])
    e2 = np.exp([0.0, 2.0, 2.0])
    want = -(np.log(e[1] / e.sum()) + np.log(e2[1] / e2.sum())) / 2
    assert abs(R.metric("multi:softprob", "mlogloss", np.array([1, 1]), mc) - want) < 1e-15
    assert R.count_of("merror", mc) == 2 and R.count_of("error", m) == 4


# ----------------------------------------------------------------------------- the comparison has teeth
@pytest.mark.parametrize("objective,metric", D.PAIRS, ids=PAIR_IDS)
def test_rejects_history_shifted_by_one_round(objective, metric):
    m, ev, refs, _ = _fit(objective, metric)
    hist = [dict(m.history[min(r + 1, len(m.history) - 1)], round=r) for r in range(len(m.history))]
    bad = R.compare_history(hist, m.train_history, refs)
    assert {"a", "b", "big"} <= _sets_of(bad), bad
    bad = R.compare_history(m.history, m.train_history[1:] + m.train_history[-1:], refs)
    assert _sets_of(bad) == {R.TRAIN}, bad
    # a round too few or too many is a violation as well
    assert R.compare_history(m.history[:-1], m.train_history, refs)
    assert R.compare_history(m.history, m.train_history[:-1], refs)


@pytest.mark.parametrize("objective,metric", D.PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("pair", [("a", "b"), ("train", "big"), ("one", "c")])
def test_rejects_swapped_columns(objective, metric, pair):
    m, ev, refs, _ = _fit(objective, metric)
    u, v = pair
    hist = copy.deepcopy(m.history)
    for rec in hist:
        rec[u], rec[v] = rec[v], rec[u]
    got = _sets_of(R.compare_history(hist, m.train_history, refs))
    # (the one-row set has five terms at the most: another set's error rate can round to its count)
    assert got == {u, v} or (u == "one" and metric in R.COUNT_METRICS and got == {v}), got


@pytest.mark.parametrize("objective,metric", D.PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", ["a", "b"])
def test_rejects_dropped_last_row(objective, metric, name):
    m, ev, refs, margins = _fit(objective, metric)
    hist = copy.deepcopy(m.history)
    for r, rec in enumerate(hist):
        rec[name] = R.metric(objective, metric, ev[name][1][:-1], margins[name][r][:-1])
    assert _sets_of(R.compare_history(hist, m.train_history, refs)) == {name}


@pytest.mark.parametrize("objective,metric", [("reg:logistic", "error"), ("reg:squarederror", "rmse"),
                                              ("reg:squarederror", "error")])
def test_rejects_dropped_last_row_past_the_grid_cap(objective, metric):
    """62 x 17 000 elements: one row of 62 out of a million terms moves rmse by more than 2^-23 of its value
    and the error count by whole units (it would drown in the logloss budget, hence these two metrics)."""
    m, ev, refs, margins = _fit_large(objective, metric)
    assert margins["large"].shape[1] * margins["large"].shape[2] > 4096 * 256
    assert R.compare_history(m.history, None, refs) == []
    hist = copy.deepcopy(m.history)
    for r, rec in enumerate(hist):
        rec["large"] = R.metric(objective, metric, ev["large"][1][:-1], margins["large"][r][:-1])
    assert _sets_of(R.compare_history(hist, None, refs)) == {"large"}
    # a single element (the last task of the last row) is visible too
    y1 = ev["large"][1].copy().reshape(-1)[:-1]
    hist = copy.deepcopy(m.history)
    for r, rec in enumerate(hist):
        m1 = margins["large"][r].reshape(-1)[:-1]
        rec["large"] = R.metric(objective, metric, y1[:, None], m1[:, None])
    assert _sets_of(R.compare_history(hist, None, refs)) == {"large"}


@pytest.mark.parametrize("objective,metric", D.PAIRS, ids=PAIR_IDS)
def test_rejects_reversed_tasks(objective, metric):
    m, ev, refs, margins = _fit(objective, metric)
    hist = copy.deepcopy(m.history)
    for r, rec in enumerate(hist):
        for name in ("a", "b", "big"):
            rec[name] = R.metric(objective, metric, ev[name][1], np.ascontiguousarray(margins[name][r][:, ::-1]))
    assert _sets_of(R.compare_history(hist, m.train_history, refs)) == {"a", "b", "big"}


def test_predict_range_matches_margins():
    """predict_range over whole rounds is the fp64 counterpart of margins_by_round."""
    m, ev, refs, margins = _fit("reg:logistic", "logloss")
    s, a, cnt = R.predict_range(m.trees, m.cuts, m.n_tasks, ev["b"][0], 0, m.trees.n_trees)
    assert cnt.tolist() == [12] * 5 and (a >= np.abs(s)).all()
    assert np.allclose(m.base_margin + s, margins["b"][-1], rtol=0, atol=13 * 2.0 ** -24 * (a.max() + 1))
    s, a, cnt = R.predict_range(m.trees, m.cuts, m.n_tasks, ev["b"][0], 7, 23)
    assert cnt.tolist() == [3, 3, 4, 3, 3]  # trees 7 .. 22: tasks 2, 3, 4, 0, 1, 2, ...
