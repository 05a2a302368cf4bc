"""``GBDT.predict_contribs`` / ``predict_leaf`` on the HIP path (csrc/gbdt_shap.hip) against fp64 Shapley values
computed from the definition (tests/_gbdt_shap_ref.py): every element inside the budget of a float32 engine.

The models are fitted on the HIP backend and the reference is built from the fitted model's own trees and cuts,
so a tree difference cannot hide behind or pose as a contribution error.  The budget and its error model are
proved on the CPU by tests/test_gbdt_shap_cpu.py.  Each test prints the worst |dev - ref| / budget it saw
(``pytest -s``)."""
import functools

import numpy as np
import pytest

import _gbdt_ref as R
import _gbdt_shap_ref as S
import _gbdt_watch_data as D
from euromillioner_amd.models import gbdt as G
from euromillioner_amd.models import gbdt_explain as E

pytestmark = pytest.mark.gpu

CONFIGS = {
    # objective, model arguments on top of D.KW, the watch sets scored
    "logistic-g0": ("reg:logistic", dict(gamma=0.0), ("one", "a", "b")),
    "logistic-g1": ("reg:logistic", dict(gamma=1.0), ("one", "a", "b")),  # leaves at internal levels
    "multi-d4": ("multi:softprob", dict(max_depth=4), ("one", "b")),  # paths that split twice on one feature
    "sqerr-d1": ("reg:squarederror", dict(max_depth=1, gamma=30.0, eta=1.0), ("one", "b")),  # d = 1, bare roots
}


@functools.lru_cache(maxsize=None)
def _sets(objective):
    return D.problem(objective)


@functools.lru_cache(maxsize=None)
def _model(name):
    objective, kw, _ = CONFIGS[name]
    m = G.GBDT(objective=objective, backend="hip", **dict(D.KW, **kw)).fit(*_sets(objective)["train"])
    assert m.backend_used == "hip"
    assert np.array_equal(m.trees.cover, m.trees.cover.astype(np.float32).astype(np.float64))  # float32 covers
    return m


@functools.lru_cache(maxsize=None)
def _ref(name, set_name, iteration_range=None):
    """(ref, budget) of a configuration on one watch set: computed once, shared, never written to."""
    m = _model(name)
    ref, bud = S.reference(m, _sets(CONFIGS[name][0])[set_name][0], iteration_range)
    ref.setflags(write=False), bud.setflags(write=False)
    return ref, bud


def _check(dev, ref, bud, what):
    assert dev.dtype == np.float32 and dev.shape == ref.shape, (dev.dtype, dev.shape, ref.shape)
    print(f"\nSHAP-RATIO {what}: worst |dev - ref| / budget = {S.worst_ratio(dev, ref, bud):.4f} "
          f"over {dev.size} values")
    assert S.violations(dev, ref, bud) == 0, (what, S.violations(dev, ref, bud), S.worst_ratio(dev, ref, bud))


CASES = [(name, s) for name, (_, _, sets) in CONFIGS.items() for s in sets]


@pytest.mark.parametrize("name,set_name", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_contribs_inside_the_budget(name, set_name):
    m = _model(name)
    X = _sets(CONFIGS[name][0])[set_name][0]
    ref, bud = _ref(name, set_name)
    dev = m.predict_contribs(X)
    assert dev.shape == (len(X), m.n_tasks, X.shape[1] + 1)
    _check(dev, ref, bud, f"{name} {set_name}")
    assert (dev[:, :, -1] == dev[:1, :, -1]).all()  # the bias does not depend on the row
    used = E.importance(m.trees, m.n_tasks, X.shape[1], "weight") > 0
    assert (dev[:, :, :-1][:, ~used] == 0).all()


def test_configurations_cover_their_cases():
    m = _model("logistic-g1")
    NN = m.trees.status.shape[1]
    assert (m.trees.status[:, :NN // 2] == 2).any()  # leaves above the last level
    m = _model("multi-d4")
    p = E.build_paths(m.trees.status, m.trees.feat, m.trees.sbin, m.trees.leaf, m.trees.cover, 4)
    depth = np.array([int(i + 1).bit_length() - 1 for i in p.node])
    assert (p.d < depth).sum() >= 5  # paths that split twice on one feature
    assert max(len(c) for c in m.cuts) == 255
    m = _model("sqerr-d1")
    roots = int((m.trees.status[:, 0] == 2).sum())
    assert 0 < roots < m.trees.n_trees  # bare root leaves: bias only


@functools.lru_cache(maxsize=None)
def _large():
    sets = D.large_problem()
    Xs, Ys = sets["small"]
    m = G.GBDT(objective="reg:logistic", backend="hip", **dict(D.KW, nround=4)).fit(Xs, Ys)
    assert m.backend_used == "hip" and m.n_tasks == 62
    return m, Xs


def test_62_tasks_600_rows():
    m, X = _large()
    bins = R.bin_features(X, m.cuts)
    ref = S.shapley(m.trees, m.trees.sbin, bins, 62, m.base_margin)
    A, N = S.magnitudes(m.trees, m.trees.sbin, bins, 62, m.base_margin)
    _check(m.predict_contribs(X), ref, S.budget(ref, A, N, m.trees.max_depth), "62 tasks x 600 rows")


def test_depth_8_paths_of_up_to_seven_features():
    """The deepest trees of the plan (the kernel's build for max_depth 6..8; 511 node slots): a numpy fit with
    its covers rounded to float32, scored on the device.  8 continuous features, so the definition's 2^|U|
    subsets stay cheap while a path crosses up to 7 distinct features."""
    rng = np.random.default_rng(21)
    X = rng.normal(size=(500, 8))
    y = np.where(X[:, 0] > 0, X[:, 1] * X[:, 2], X[:, 3] + X[:, 4] * X[:, 5]) + np.abs(X[:, 6]) * X[:, 7]
    m = G.GBDT(objective="reg:squarederror", backend="numpy", **dict(D.KW, max_depth=8, nround=3)).fit(X[:400], y[:400])
    S.round_covers(m.trees)
    p = E.build_paths(m.trees.status, m.trees.feat, m.trees.sbin, m.trees.leaf, m.trees.cover, 8)
    assert p.d.max() >= 6 and (np.bincount(p.d)[2:6] > 0).all()
    ref, bud = S.reference(m, X[400:])
    _check(m.predict_contribs(X[400:], backend="hip"), ref, bud, "depth 8")
    assert np.array_equal(m.predict_leaf(X[400:], backend="hip"), E.leaf_index_numpy(m, X[400:]))


def test_iteration_range():
    m = _model("logistic-g0")
    X = _sets("reg:logistic")["b"][0]
    ref, bud = _ref("logistic-g0", "b", (3, 9))
    dev = m.predict_contribs(X, iteration_range=(3, 9))
    _check(dev, ref, bud, "rounds [3, 9)")
    assert np.abs(dev - m.predict_contribs(X)).max() > 1e-3


def test_chunks_and_runs_are_bit_identical():
    m = _model("logistic-g1")
    X = _sets("reg:logistic")["b"][0]
    base = m.predict_contribs(X)
    assert np.array_equal(base, m.predict_contribs(X))  # two runs
    for chunk in (1, 100, 256):
        assert np.array_equal(base, m.predict_contribs(X, chunk_rows=chunk)), chunk
    m62, X62 = _large()
    assert np.array_equal(m62.predict_contribs(X62), m62.predict_contribs(X62, chunk_rows=100))


@pytest.mark.parametrize("name", ["logistic-g1", "multi-d4"])
def test_additivity_against_the_engines_margin(name):
    m = _model(name)
    X = _sets(CONFIGS[name][0])["b"][0]
    _, bud = _ref(name, "b")
    dev = m.predict_contribs(X).astype(np.float64)
    margin = m.predict_margin(X, backend="hip")
    err = np.abs(dev.sum(axis=2) - margin)
    tol = bud.sum(axis=2)
    print(f"\nSHAP-RATIO additivity {name}: worst |sum(phi) - margin| / tolerance = {(err / tol).max():.4f}")
    assert (err <= tol).all()


@pytest.mark.parametrize("name", ["logistic-g1", "multi-d4", "sqerr-d1"])
def test_predict_leaf_equals_the_numpy_walk(name):
    m = _model(name)
    X = _sets(CONFIGS[name][0])["b"][0]
    dev = m.predict_leaf(X)
    assert dev.dtype == np.int32 and dev.shape == (len(X), m.trees.n_trees)
    assert np.array_equal(dev, E.leaf_index_numpy(m, X))
    assert np.array_equal(dev[:5], S.heap_walk(m.trees, m.trees.sbin, R.bin_features(X[:5], m.cuts)))


@pytest.mark.parametrize("name", ["logistic-g1", "multi-d4"])
def test_loaded_checkpoint_is_bit_identical_on_the_device(name, tmp_path):
    m = _model(name)
    X = _sets(CONFIGS[name][0])["b"][0]
    m.save(str(tmp_path / "m.json"))
    ld = G.GBDT.load(str(tmp_path / "m.json"))
    assert ld.cuts is None and ld.backend_used == "numpy"
    assert np.array_equal(ld.predict_contribs(X, backend="hip"), m.predict_contribs(X))
    assert np.array_equal(ld.predict_leaf(X, backend="hip"), m.predict_leaf(X))


def test_outside_the_plan_falls_back_to_numpy():
    from euromillioner_amd.models import gbdt_hip

    # max_depth 9 on a tiny set
    X, y = _sets("multi:softprob")["c"]
    deep = G.GBDT(objective="multi:softprob", backend="numpy", **dict(D.KW, max_depth=9, nround=2)).fit(X, y)
    # more features than the LDS tile holds
    rng = np.random.default_rng(5)
    Xw = rng.integers(0, 3, size=(120, 600)).astype(np.float64)
    yw = Xw[:, 7] - Xw[:, 450] + 0.1 * rng.normal(size=120)
    wide = G.GBDT(objective="reg:squarederror", backend="numpy", **dict(D.KW, max_depth=2, nround=3)).fit(Xw, yw)
    for m, x in ((deep, X), (wide, Xw)):
        with pytest.raises(gbdt_hip.PlanUnsupported):
            m.predict_contribs(x, backend="hip")
        want = E.contribs_numpy(m, x).astype(np.float32)
        assert np.array_equal(m.predict_contribs(x, backend="auto"), want)
        m.backend_used = "hip"  # as after a device fit
        assert np.array_equal(m.predict_contribs(x), want)
    # the leaf index has no LDS tile: the wide model runs on the device
    assert np.array_equal(wide.predict_leaf(Xw, backend="hip"), E.leaf_index_numpy(wide, Xw))
