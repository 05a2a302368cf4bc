"""``RandomForest.predict_contribs`` / ``apply`` on the HIP path (csrc/forest_shap.hip) against fp64 Shapley values
computed from the definition (tests/_rf_shap_ref.py): every element of every case inside the budget of a float32
engine.

The forests are the numpy engine's, so a fit difference cannot hide behind or pose as a contribution error.  The
budget and its error model are proved on the CPU by tests/test_rf_shap_cpu.py.  Each test prints the worst
|dev - ref| / budget it saw (``pytest -s``)."""
import contextlib
import functools

import numpy as np
import pytest

import _rf_shap_ref as R
from euromillioner_amd.models import forest_explain as E
from euromillioner_amd.models.forest import RandomForest

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _auto(rf):
    """The shared forests were fitted with device="cpu"; inside, the forest is as one fitted or loaded on a GPU box."""
    rf.device = "auto"
    try:
        yield rf
    finally:
        rf.device = "cpu"


def _check(dev, ref, bud, what):
    assert dev.dtype == np.float32 and dev.shape == ref.shape, (dev.dtype, dev.shape, ref.shape)
    print(f"\nRF-SHAP-RATIO {what}: worst |dev - ref| / budget = {R.worst_ratio(dev, ref, bud):.4f} "
          f"over {dev.size} values")
    assert R.violations(dev, ref, bud) == 0, (what, R.violations(dev, ref, bud), R.worst_ratio(dev, ref, bud))
    assert (dev[bud == 0] == 0).all()  # a column no path crosses is exactly 0


@pytest.mark.parametrize("name", list(R.CASES))
def test_contribs_inside_the_budget(name):
    rf, X, ref, bud = R.build_case(name)
    dev = rf.predict_contribs(X, backend="hip")
    assert dev.shape == (len(X), 62, rf.F + 1)
    _check(dev, ref, bud, name)
    assert (dev[:, :, -1] == dev[:1, :, -1]).all()  # the bias does not depend on the row
    with _auto(rf):
        assert np.array_equal(dev, rf.predict_contribs(X))  # backend=None picks the device inside the plan
    if name == "d3":
        a = R.shapley_trees(rf, X)  # reference (a): the tree-level definition
        assert R.violations(dev, a, bud) == 0
    if name == "d0":
        assert (dev[:, :, :-1] == 0).all()
        mean_root = np.asarray(rf.value, np.float64)[:, 0, :62].mean(axis=0)
        assert np.abs(dev[0, :, -1] - mean_root).max() <= 2.0 ** -23


def test_cases_cover_their_shapes():
    p = E.paths_of(R.build_case("d8")[0])
    assert p.d.max() == 8 and len(p.d) % 64 != 0 and len(p.d) > 64
    p = E.paths_of(R.build_case("minleaf")[0])
    assert (np.bincount(p.d, minlength=9)[1:] > 0).all()
    assert len(R.build_case("d3")[1]) == 2 * 64 + 2 + 2


@pytest.mark.parametrize("name", ["d3", "minleaf", "lags2"])
def test_chunks_and_runs_are_bit_identical(name):
    rf, X, _, _ = R.build_case(name)
    base = rf.predict_contribs(X, backend="hip")
    assert np.array_equal(base, rf.predict_contribs(X, backend="hip"))  # two runs
    for chunk in (1, 64, 100):
        assert np.array_equal(base, rf.predict_contribs(X, backend="hip", chunk_rows=chunk)), chunk
    dev = rf.predict_contribs_device(X)
    assert dev.is_cuda and dev.dtype.is_floating_point and tuple(dev.shape) == base.shape
    assert np.array_equal(dev.cpu().numpy(), base)


@pytest.mark.parametrize("name", ["d8", "lags2"])
def test_loaded_forest_is_bit_identical_on_the_device(name, tmp_path):
    rf, X, _, _ = R.build_case(name)
    rf.save(str(tmp_path / "f.npz"))
    ld = RandomForest.load(str(tmp_path / "f.npz"))
    assert np.array_equal(ld.predict_contribs(X, backend="hip"), rf.predict_contribs(X, backend="hip"))
    assert np.array_equal(ld.apply(X, backend="hip"), rf.apply(X, backend="hip"))


@pytest.mark.parametrize("name", ["d8", "minleaf", "lags4"])
def test_additivity_against_the_engines_proba(name):
    rf, X, _, bud = R.build_case(name)
    dev = rf.predict_contribs(X, backend="hip").astype(np.float64)
    proba = rf.predict_proba_device(np.array(X))[:, :62].cpu().numpy().astype(np.float64)
    err = np.abs(dev.sum(axis=2) - proba)
    tol = bud.sum(axis=2)
    print(f"\nRF-SHAP-RATIO additivity {name}: worst |sum(phi) - proba| / tolerance = {(err / tol).max():.4f}")
    assert (err <= tol).all()


@functools.lru_cache(maxsize=None)
def _deep():
    """A depth-9 forest: outside the contribution plan, inside the leaf-index kernel's."""
    _, X, _, _ = R.build_case("d3")
    Xf, Y, F = R.data(1)
    rf = RandomForest(n_trees=3, max_depth=9, seed=11, device="cpu").fit(Xf[:3000], Y[:3000], F)
    assert E.paths_of(rf).d.max() == 9
    return rf, np.array(X)


@pytest.mark.parametrize("name", list(R.CASES) + ["deep"])
def test_apply_equals_the_numpy_walk(name):
    rf, X = _deep() if name == "deep" else R.build_case(name)[:2]
    dev = rf.apply(X, backend="hip")
    assert dev.dtype == np.int32 and dev.shape == (len(X), len(rf.feat))
    assert np.array_equal(dev, E.apply_numpy(rf, X))
    assert np.array_equal(dev[:5], R.heap_walk(rf, X[:5]))
    with _auto(rf):
        assert np.array_equal(dev, rf.apply(X))


def test_outside_the_plan_falls_back_to_numpy():
    rf, X = _deep()
    with pytest.raises(ValueError):
        rf.predict_contribs(X, backend="hip")
    with pytest.raises(ValueError):
        rf.predict_contribs_device(X)
    want = E.contribs_numpy(rf, X).astype(np.float32)
    with _auto(rf):
        assert np.array_equal(rf.predict_contribs(X), want)
