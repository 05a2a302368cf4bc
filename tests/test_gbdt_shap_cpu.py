"""GBDT explanations on the numpy backend: ``predict_contribs`` against Shapley values from the definition
(tests/_gbdt_shap_ref.py), the budget of a float32 engine proved on a float32 emulation and on planted
mistakes, ``predict_leaf``, ``get_score``, loaded checkpoints, validation, and ``euromillioner explain``."""
import functools
import json
import math

import numpy as np
import pytest

import _gbdt_ref as R
import _gbdt_shap_ref as S
import _gbdt_watch_data as D
from euromillioner_amd.models import gbdt as G
from euromillioner_amd.models import gbdt_explain as E

CONFIGS = {
    "logistic-g0": ("reg:logistic", dict(gamma=0.0)),
    "logistic-bs": ("reg:logistic", dict(gamma=0.0, base_score=0.3)),  # a non-zero base margin
    "logistic-g1": ("reg:logistic", dict(gamma=1.0)),  # pruning leaves leaves at internal levels
    "multi-d4": ("multi:softprob", dict(max_depth=4)),  # continuous features: paths that split twice on one
    "sqerr-d1": ("reg:squarederror", dict(max_depth=1, gamma=30.0, eta=1.0)),  # d = 1 and bare root leaves
}


@functools.lru_cache(maxsize=None)
def _sets(objective):
    return D.problem(objective)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, X, bins, ref, budget): a numpy fit with float32 covers, scored on the 257 rows of set ``b``."""
    objective, kw = CONFIGS[name]
    m = G.GBDT(objective=objective, backend="numpy", **dict(D.KW, **kw)).fit(*_sets(objective)["train"])
    S.round_covers(m.trees)
    X = _sets(objective)["b"][0]
    ref, bud = S.reference(m, X)
    return m, X, R.bin_features(X, m.cuts), ref, bud


def _emulate(m, bins, dtype=np.float32, mistake=None, k0=0, k1=None):
    """The path formula with every value and operation in ``dtype`` (leaf by leaf, feature by feature, in the
    order of the module docstring of gbdt_explain), optionally with one planted mistake."""
    tr, T = m.trees, m.n_tasks
    f_ = dtype
    n, F = bins.shape
    out = np.zeros((n, T, F + 1), dtype=dtype)
    if mistake != "no_base":
        out[:, :, F] = f_(m.base_margin)
    first_edge = True
    for k in range(k0, tr.n_trees if k1 is None else k1):
        t = (k + 1) % T if mistake == "task" else k % T
        for i in np.nonzero(tr.status[k] == 2)[0]:
            i = int(i)
            depth = (i + 1).bit_length() - 1
            fs, lo, hi, z = [], [], [], []
            for lvl in range(depth):
                p, c = ((i + 1) >> (depth - lvl)) - 1, ((i + 1) >> (depth - lvl - 1)) - 1
                f, b = int(tr.feat[k, p]), int(tr.sbin[k, p])
                if f not in fs:
                    fs.append(f), lo.append(-1), hi.append(np.inf), z.append(f_(1))
                j = fs.index(f)
                if c == 2 * p + 2:
                    lo[j] = max(lo[j], b)
                else:
                    hi[j] = min(hi[j], b)
                zz = f_(f_(tr.cover[k, c]) / f_(tr.cover[k, p]))
                if mistake == "one_minus_z" and first_edge:
                    zz, first_edge = f_(1) - zz, False
                z[j] = f_(z[j] * zz)
            d = len(fs)
            lv = f_(tr.leaf[k, i])
            zp = f_(1)
            for j in range(d):
                zp = f_(zp * z[j])
            out[:, t, F] += f_(lv * zp)
            if mistake == "ge_lo":
                o = [((bins[:, f] >= lo[j]) & (bins[:, f] <= hi[j])).astype(dtype) for j, f in enumerate(fs)]
            else:
                o = [((bins[:, f] > lo[j]) & (bins[:, f] <= hi[j])).astype(dtype) for j, f in enumerate(fs)]
            for a in range(d):
                c = [np.ones(n, dtype)] + [np.zeros(n, dtype) for _ in range(d - 1)]
                deg = 0
                for j in range(d):
                    if j == a:
                        continue
                    for s in range(deg + 1, 0, -1):
                        c[s] = c[s] * z[j] + c[s - 1] * o[j]
                    c[0] = c[0] * z[j]
                    deg += 1
                w = np.zeros(n, dtype)
                for s in range(d):
                    ws = 1.0 / d if mistake == "flat_weights" else \
                        math.factorial(s) * math.factorial(d - 1 - s) / math.factorial(d)
                    w = w + f_(ws) * c[s]
                out[:, t, fs[a]] += lv * (o[a] - z[a]) * w
    assert out.dtype == dtype
    return out


# ----------------------------------------------------------------------------- the formula against the definition
@pytest.mark.parametrize("name", list(CONFIGS))
def test_contribs_match_the_definition(name):
    m, X, bins, ref, _ = _case(name)
    phi = E.contribs_numpy(m, X)
    assert phi.shape == ref.shape == (len(X), m.n_tasks, X.shape[1] + 1) and phi.dtype == np.float64
    scale = np.abs(ref).max()
    assert np.abs(phi - ref).max() <= 1e-12 * scale, np.abs(phi - ref).max()
    # additivity, the constant bias column, exact zeros on unused features
    margin = m.predict_margin(X, backend="numpy")
    assert np.abs(phi.sum(axis=2) - margin).max() <= 1e-12 * max(1.0, np.abs(margin).max())
    assert (phi[:, :, -1] == phi[:1, :, -1]).all()
    used = E.importance(m.trees, m.n_tasks, X.shape[1], "weight") > 0
    assert name == "multi-d4" or not used.all()
    assert (phi[:, :, :-1][:, ~used] == 0).all()
    out = m.predict_contribs(X)
    assert out.dtype == np.float32 and np.array_equal(out, phi.astype(np.float32))


def test_configurations_cover_their_cases():
    """The cases the configurations are there for do occur."""
    m = _case("logistic-g1")[0]
    NN = m.trees.status.shape[1]
    assert (m.trees.status[:, :NN // 2] == 2).any()  # leaves above the last level
    m = _case("multi-d4")[0]
    paths = E.build_paths(m.trees.status, m.trees.feat, m.trees.sbin, m.trees.leaf, m.trees.cover, 4)
    depth = np.array([int(i + 1).bit_length() - 1 for i in paths.node])
    assert (paths.d < depth).sum() >= 5  # paths that split twice on one feature
    m = _case("sqerr-d1")[0]
    roots = int((m.trees.status[:, 0] == 2).sum())
    assert 0 < roots < m.trees.n_trees  # bare root leaves: bias only


def test_iteration_range():
    m, X, bins, _, _ = _case("logistic-g0")
    T = m.n_tasks
    ref = S.shapley(m.trees, m.trees.sbin, bins, T, m.base_margin, 3 * T, 9 * T)
    phi = E.contribs_numpy(m, X, iteration_range=(3, 9))
    assert np.abs(phi - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(phi - E.contribs_numpy(m, X)).max() > 1e-3
    with pytest.raises(ValueError):
        E.contribs_numpy(m, X, iteration_range=(3, 13))


# ----------------------------------------------------------------------------- the budget
@pytest.mark.parametrize("name", list(CONFIGS))
def test_budget_holds_for_a_float32_engine(name):
    m, X, bins, ref, bud = _case(name)
    dev = _emulate(m, bins, np.float32)
    print(f"\nSHAP-RATIO float32 emulation {name}: worst |dev - ref| / budget = {S.worst_ratio(dev, ref, bud):.4f}")
    assert S.violations(dev, ref, bud) == 0
    assert np.abs(_emulate(m, bins, np.float64) - ref).max() <= 1e-12 * np.abs(ref).max()
    # a float32 budget: far below the size of the values it guards
    assert bud.max() < 1e-4 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("mistake", ["ge_lo", "one_minus_z", "flat_weights", "no_base", "task"])
def test_budget_rejects_planted_mistakes(mistake):
    m, X, bins, ref, bud = _case("logistic-bs")
    assert abs(m.base_margin) > 0.5
    dev = _emulate(m, bins, np.float32, mistake=mistake)
    err = np.abs(dev.astype(np.float64) - ref)
    assert (err > 10 * bud).any(), mistake
    assert S.violations(dev, ref, bud) > 0


# ----------------------------------------------------------------------------- leaf indices
@pytest.mark.parametrize("name", ["logistic-g1", "multi-d4"])
def test_predict_leaf_is_the_heap_walk(name):
    m, X, bins, _, _ = _case(name)
    got = m.predict_leaf(X[:40])
    assert got.dtype == np.int32 and got.shape == (40, m.trees.n_trees)
    assert np.array_equal(got, S.heap_walk(m.trees, m.trees.sbin, bins[:40]))
    assert (m.trees.status[np.arange(m.trees.n_trees)[None, :], got] == 2).all()


# ----------------------------------------------------------------------------- importances
def _hand_model():
    """Two trees of depth 2 over 3 features, one task: tree 0 splits on f0 then f2 (left) and f0 (right),
    tree 1 on f2 only."""
    tr = G.TreeArrays(2, 2)
    tr.status[0] = [1, 1, 1, 2, 2, 2, 2]
    tr.feat[0, :3] = [0, 2, 0]
    tr.gain[0, :3] = [8.0, 2.0, 1.0]
    tr.cover[0] = [10.0, 6.0, 4.0, 3.0, 3.0, 1.0, 3.0]
    tr.split_value[0, :3] = [0.5, 1.5, 2.5]
    tr.leaf[0, 3:] = [0.1, -0.2, 0.3, 0.4]
    tr.status[1, :3] = [1, 2, 2]
    tr.feat[1, 0] = 2
    tr.gain[1, 0] = 4.0
    tr.cover[1, :3] = [10.0, 5.0, 5.0]
    tr.split_value[1, 0] = 0.5
    tr.leaf[1, 1:3] = [-0.5, 0.5]
    m = G.GBDT(objective="reg:squarederror", max_depth=2, nround=2, backend="numpy")
    m.trees, m.n_tasks, m.num_feature, m.backend_used = tr, 1, 3, "numpy"
    return m


def test_get_score_hand_sums():
    m = _hand_model()
    assert m.get_score("weight") == {"f0": 2.0, "f2": 2.0}
    assert m.get_score("total_gain") == {"f0": 9.0, "f2": 6.0}
    assert m.get_score("gain") == {"f0": 4.5, "f2": 3.0}
    assert m.get_score("total_cover") == {"f0": 14.0, "f2": 16.0}
    assert m.get_score("cover") == {"f0": 7.0, "f2": 8.0}
    pt = m.get_score("total_gain", per_task=True)
    assert pt.dtype == np.float64 and np.array_equal(pt, [[9.0, 0.0, 6.0]])
    with pytest.raises(ValueError):
        m.get_score("splits")
    # two tasks: tree 0 -> task 0, tree 1 -> task 1; the dict sums the tasks, gain averages over all splits
    m.n_tasks = 2
    assert np.array_equal(m.get_score("weight", per_task=True), [[2.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    assert np.array_equal(m.get_score("gain", per_task=True), [[4.5, 0.0, 2.0], [0.0, 0.0, 4.0]])
    assert m.get_score("gain") == {"f0": 4.5, "f2": 3.0}


def test_hand_model_contribs_from_split_values():
    """A model with split values only (as a loaded one): cuts and sbin are derived, the walk is x < value."""
    m = _hand_model()
    X = np.array([[0.0, 9.0, 0.0], [0.5, 9.0, 1.5], [3.0, 9.0, 0.4], [2.5, 9.0, 2.0], [0.4, 9.0, 1.6]])
    cuts, sbin = E.model_bins(m)
    assert [c.tolist() for c in cuts] == [[0.5, 2.5], [], [0.5, 1.5]]
    bins = R.bin_features(X, cuts)
    assert np.array_equal(m.predict_leaf(X), S.heap_walk(m.trees, sbin, bins))
    assert m.predict_leaf(X).tolist() == [[3, 1], [5, 2], [6, 1], [6, 2], [4, 2]]
    phi = E.contribs_numpy(m, X)
    ref = S.shapley(m.trees, sbin, bins, 1, m.base_margin)
    assert np.abs(phi - ref).max() <= 1e-14
    margin = m.predict_margin(X)  # the raw-value walk
    assert np.abs(phi.sum(axis=2) - margin).max() <= 1e-14
    assert (phi[:, 0, 1] == 0).all()


# ----------------------------------------------------------------------------- checkpoints and validation
@pytest.mark.parametrize("name", ["logistic-g1", "multi-d4"])
def test_loaded_checkpoint_explains_like_the_fitted_model(name, tmp_path):
    m, X, _, _, _ = _case(name)
    m.save(str(tmp_path / "m.json"))
    ld = G.GBDT.load(str(tmp_path / "m.json"))
    assert ld.cuts is None
    assert np.array_equal(ld.predict_leaf(X), m.predict_leaf(X))
    a, b = E.contribs_numpy(ld, X), E.contribs_numpy(m, X)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert ld.get_score("total_gain") == m.get_score("total_gain")


def _broken(tmp_path, edit):
    m = _hand_model()
    m.save(str(tmp_path / "m.json"))
    with open(tmp_path / "m.json", encoding="utf-8") as f:
        d = json.load(f)
    edit(d["learner"]["gradient_booster"]["model"]["trees"][0]["nodes"])
    with open(tmp_path / "bad.json", "w", encoding="utf-8") as f:
        json.dump(d, f)
    return G.GBDT.load(str(tmp_path / "bad.json"))


@pytest.mark.parametrize("what", ["feat", "child", "cover", "orphan"])
def test_bad_checkpoints_raise(what, tmp_path):
    def edit(nodes):
        by_id = {nd["nodeid"]: nd for nd in nodes}
        if what == "feat":
            by_id[1]["split"] = "f3"  # F = 3
        elif what == "child":
            nodes.remove(by_id[4])
        elif what == "cover":
            by_id[2]["cover"] = 0.0
        else:
            by_id[1].pop("split"), by_id[1].pop("split_condition")
            by_id[1]["leaf"] = 0.25  # node 1 a leaf, its children still there

    ld = _broken(tmp_path, edit)
    X = np.zeros((2, 3))
    for call in (lambda: ld.predict_contribs(X), lambda: ld.predict_leaf(X)):
        with pytest.raises(ValueError):
            call()


# ----------------------------------------------------------------------------- the command line
def test_explain_cli_finds_the_planted_drivers(tmp_path, capsys):
    """``euromillioner explain`` on a checkpoint trained on planted data (planted = 0.9): number j drives
    ``perm[j]``, so the top feature of a picked number m must be the number the permutation maps to m.
    Achieved on the numpy backend with 700 draws, seed 4, 8 rounds: 5 of the 5 picked main numbers (the test
    asks for at least 4)."""
    from euromillioner_amd import cli
    from euromillioner_amd.data.draws import DrawSet

    ck = str(tmp_path / "gbdt.json")
    data = ["--data-source", "synthetic", "--n-draws", "700", "--seed", "4", "--planted", "0.9", "--device", "cpu"]
    assert cli.main(["train", "--model", "gbdt", "--nround", "8", "--gamma", "0", "--ckpt", ck] + data) == 0
    capsys.readouterr()
    assert cli.main(["explain", "--ckpt", ck, "--top", "2"] + data) == 0
    out = capsys.readouterr().out.strip().splitlines()
    res = json.loads(out[-1])
    assert len(out) == 8 and all(":" in ln for ln in out[:7])
    assert res["model"] == "gbdt" and res["backend"] == "numpy" and len(res["explain"]) == 7
    assert all(len(p["top"]) == 2 for p in res["explain"])
    perm = np.asarray(DrawSet.synthetic(n=700, seed=4, planted=0.9).meta["perm"])
    hits = 0
    for m, p in zip(res["main"], res["explain"][:5]):
        assert p["pick"] == f"number {m}"
        driver = int(np.nonzero(perm[:50] == m)[0][0]) + 1
        hits += p["top"][0]["feature"] == f"number {driver}"
    print(f"\nEXPLAIN planted drivers found: {hits} of 5")
    assert hits >= 4
    # other checkpoints: exit code 3
    other = tmp_path / "model.zip"
    other.write_bytes(b"")
    assert cli.main(["explain", "--ckpt", str(other)] + data) == 3
