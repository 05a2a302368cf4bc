"""Forest explanations on the numpy backend: ``RandomForest.predict_contribs`` against Shapley values from the
definition (tests/_rf_shap_ref.py), the budget of a float32 engine proved on a float32 emulation and on planted
mistakes, ``apply``, saved forests, validation, and ``euromillioner explain`` on a forest checkpoint."""
import json
import math

import numpy as np
import pytest

import _rf_shap_ref as R
from euromillioner_amd.models import forest_explain as E
from euromillioner_amd.models.forest import RandomForest


def _emulate(rf, X, dtype=np.float32, mistake=None):
    """The path formula with every value and operation in ``dtype``, leaf by leaf and feature by feature in table
    order (the bias in fp64, as the device sums it), optionally with one planted mistake."""
    f_ = dtype
    feat, cover = np.asarray(rf.feat), np.asarray(rf.cover, np.float32)
    bits = R.bits_of(X, rf.F)
    n, F, T = len(bits), rf.F, len(feat)
    out = np.zeros((n, R.N_OUT, F + 1), dtype=dtype)
    bias = np.zeros(R.N_OUT)
    for t, i, path in R.leaf_paths(feat, cover):
        d = len(path)
        v = np.asarray(rf.value[t, i, :R.N_OUT], dtype=dtype)
        z, o = [], []
        for lvl, (f, side, _) in enumerate(path):
            p = ((i + 1) >> (d - lvl)) - 1
            c = 2 * p + 1 + (side if mistake != "z_sibling" else 1 - side)
            z.append(f_(f_(cover[t, c]) / f_(cover[t, p])))
            o.append((bits[:, f] == (side if mistake != "sides" else 1 - side)).astype(dtype))
        bias += rf.value[t, i, :R.N_OUT].astype(np.float64) * float(np.prod([zj for _, _, zj in path]))
        players = list(range(d - 1)) if mistake == "dropped" and d > 1 else list(range(d))
        dd = len(players)
        for a in players:
            c = [np.ones(n, dtype)] + [np.zeros(n, dtype) for _ in range(dd - 1)]
            deg = 0
            for j in players:
                if j == a:
                    continue
                for s in range(deg + 1, 0, -1):
                    c[s] = c[s] * z[j] + c[s - 1] * o[j]
                c[0] = c[0] * z[j]
                deg += 1
            w = np.zeros(n, dtype)
            for s in range(dd):
                if mistake == "weights_d_minus_1" and dd > 1:
                    ws = math.factorial(s) * math.factorial(dd - 2 - s) / math.factorial(dd - 1) if s < dd - 1 else 0.0
                else:
                    ws = math.factorial(s) * math.factorial(dd - 1 - s) / math.factorial(dd)
                w = w + f_(ws) * c[s]
            out[:, :, path[a][0]] += ((o[a] - z[a]) * w)[:, None] * v[None, :]
    if mistake != "no_1_over_T":
        out = out / f_(T)
        bias = bias / T
    out[:, :, F] = bias.astype(dtype)[None, :]
    assert out.dtype == dtype
    return out


# ----------------------------------------------------------------------------- the two references, the formula
@pytest.mark.parametrize("name", ["d3", "d1", "d0"])
def test_tree_level_definition_equals_the_leaf_games(name):
    rf, X, ref, _ = R.build_case(name)
    a = R.shapley_trees(rf, X)
    assert a.shape == ref.shape
    assert np.abs(a - ref).max() <= 1e-14, np.abs(a - ref).max()


@pytest.mark.parametrize("name", list(R.CASES))
def test_numpy_specification_inside_the_budget(name):
    rf, X, ref, bud = R.build_case(name)
    phi = E.contribs_numpy(rf, X)
    assert phi.shape == ref.shape == (len(X), 62, rf.F + 1) and phi.dtype == np.float64
    assert np.abs(phi - ref).max() <= 1e-13
    out = rf.predict_contribs(X, backend="numpy")
    assert out.dtype == np.float32 and np.array_equal(out, phi.astype(np.float32))
    print(f"\nRF-SHAP-RATIO numpy {name}: worst |spec - ref| / budget = {R.worst_ratio(out, ref, bud):.4f}")
    assert R.violations(out, ref, bud) == 0
    assert (out[bud == 0] == 0).all()
    assert (out[:, :, -1] == out[:1, :, -1]).all()  # the bias does not depend on the row
    # additivity against an fp64 predict_proba
    assert np.abs(phi.sum(axis=2) - R.proba64(rf, X)).max() <= 1e-13
    assert np.abs(out.astype(np.float64).sum(axis=2) - rf.predict_proba(X)).max() <= 1e-5


def test_cases_cover_their_shapes():
    p = E.paths_of(R.build_case("d8")[0])
    assert p.d.max() == 8 and len(p.d) % 64 != 0
    p = E.paths_of(R.build_case("minleaf")[0])
    assert (np.bincount(p.d, minlength=9)[1:] > 0).all()  # leaves at every depth from 1 to 8
    rf, X, ref, _ = R.build_case("d0")
    assert (E.paths_of(rf).d == 0).all() and (ref[:, :, :-1] == 0).all()
    assert np.abs(ref[0, :, -1] - np.asarray(rf.value, np.float64)[:, 0, :62].mean(axis=0)).max() <= 1e-15
    assert R.build_case("lags4")[0].F == 248 and R.build_case("lags2")[0].F == 124
    X = R.build_case("d3")[1]
    assert len(X) == 132 and X[-2, 0] == 0 and X[-1, 0] == (1 << 62) - 1


# ----------------------------------------------------------------------------- the budget
@pytest.mark.parametrize("name", list(R.CASES))
def test_budget_holds_for_a_float32_engine(name):
    rf, X, ref, bud = R.build_case(name)
    dev = _emulate(rf, X, np.float32)
    print(f"\nRF-SHAP-RATIO float32 emulation {name}: worst |dev - ref| / budget = {R.worst_ratio(dev, ref, bud):.4f}")
    assert R.violations(dev, ref, bud) == 0
    assert np.abs(_emulate(rf, X, np.float64) - ref).max() <= 1e-13
    assert bud.max() < 1e-4  # a float32 budget: far below the probabilities it guards


@pytest.mark.parametrize("mistake", ["sides", "z_sibling", "no_1_over_T", "dropped", "weights_d_minus_1"])
def test_budget_rejects_planted_mistakes(mistake):
    rf, X, ref, bud = R.build_case("minleaf")
    dev = _emulate(rf, X, np.float32, mistake=mistake)
    err = np.abs(dev.astype(np.float64) - ref)
    assert (err > 10 * bud).any(), mistake
    assert R.violations(dev, ref, bud) > 0


# ----------------------------------------------------------------------------- leaf indices, persistence
@pytest.mark.parametrize("name", ["d3", "minleaf", "lags2", "d0"])
def test_apply_is_the_row_at_a_time_walk(name):
    rf, X, _, _ = R.build_case(name)
    got = rf.apply(X, backend="numpy")
    assert got.dtype == np.int32 and got.shape == (len(X), len(rf.feat))
    assert np.array_equal(got, R.heap_walk(rf, X))
    assert (np.asarray(rf.feat)[np.arange(len(rf.feat))[None, :], got] < 0).all()


def test_saved_forest_explains_identically(tmp_path):
    rf, X, _, _ = R.build_case("lags2")
    rf.save(str(tmp_path / "f.npz"))
    ld = RandomForest.load(str(tmp_path / "f.npz"))
    ld.device = "cpu"
    assert np.array_equal(ld.predict_contribs(X, backend="numpy"), rf.predict_contribs(X, backend="numpy"))
    assert np.array_equal(ld.apply(X, backend="numpy"), rf.apply(X, backend="numpy"))


# ----------------------------------------------------------------------------- validation
def _hand_forest(feat, cover):
    rf = RandomForest(n_trees=1, max_depth=2, device="cpu")
    rf.F, rf.k = 62, 8
    rf.feat = np.array([feat], dtype=np.int16)
    rf.cover = np.array([cover], dtype=np.float32)
    rf.value = np.zeros((1, 7, 64), dtype=np.float32)
    rf.value[0, :, :62] = np.linspace(0.0, 1.0, 7)[:, None]
    rf.gain = np.zeros((1, 7))
    return rf


def test_hand_forest_and_validation_errors():
    X = np.array([[0], [1 << 3], [(1 << 3) | (1 << 5)]], dtype=np.uint64)
    good = _hand_forest([3, 5, -1, -1, -1, -2, -2], [10, 6, 4, 3, 3, 0, 0])
    assert good.apply(X).tolist() == [[3], [2], [2]]
    phi = E.contribs_numpy(good, X)
    assert np.abs(phi - R.shapley_leaves(good, X, with_budget=False)).max() <= 1e-15
    assert np.abs(phi - R.shapley_trees(good, X)).max() <= 1e-15
    bad = {
        "a repeated path feature": _hand_forest([3, 3, -1, -1, -1, -2, -2], [10, 6, 4, 3, 3, 0, 0]),
        "a zero cover": _hand_forest([3, 5, -1, -1, -1, -2, -2], [10, 0, 4, 3, 3, 0, 0]),
        "feat == F": _hand_forest([3, 62, -1, -1, -1, -2, -2], [10, 6, 4, 3, 3, 0, 0]),
        "feat < -2": _hand_forest([3, 5, -1, -3, -1, -2, -2], [10, 6, 4, 3, 3, 0, 0]),
    }
    for what, rf in bad.items():
        for call in (lambda: rf.predict_contribs(X), lambda: rf.apply(X)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        good.predict_contribs(X, backend="cuda")
    with pytest.raises(ValueError):
        good.predict_contribs(np.zeros((2, 0), dtype=np.uint64))


# ----------------------------------------------------------------------------- the command line
def test_explain_cli_on_a_forest_finds_the_planted_drivers(tmp_path, capsys):
    """``euromillioner explain`` on a forest checkpoint trained on planted data (planted = 0.9): number j drives
    ``perm[j]``, so the top feature of a picked number m must be the number the permutation maps to m.
    Achieved on the numpy backend with 1500 draws, seed 4, 30 trees of depth 6: 5 of the 5 picked main numbers
    (the test asks for most of them: at least 3)."""
    from euromillioner_amd import cli
    from euromillioner_amd.data.draws import DrawSet

    ck = str(tmp_path / "forest.npz")
    data = ["--data-source", "synthetic", "--n-draws", "1500", "--seed", "4", "--planted", "0.9", "--device", "cpu"]
    assert cli.main(["train", "--model", "rf", "--trees", "30", "--rf-max-depth", "6", "--ckpt", ck] + data) == 0
    capsys.readouterr()
    assert cli.main(["explain", "--ckpt", ck, "--top", "2"] + data) == 0
    out = capsys.readouterr().out.strip().splitlines()
    res = json.loads(out[-1])
    assert len(out) == 8 and all(":" in ln for ln in out[:7])
    assert res["model"] == "rf" and res["backend"] == "numpy" and len(res["explain"]) == 7
    assert all(len(p["top"]) == 2 and {"pick", "proba", "bias", "top"} <= set(p) for p in res["explain"])
    assert {"main", "stars", "after_draw"} <= set(res)
    perm = np.asarray(DrawSet.synthetic(n=1500, seed=4, planted=0.9).meta["perm"])
    hits = 0
    for m, p in zip(res["main"], res["explain"][:5]):
        assert p["pick"] == f"number {m}"
        driver = int(np.nonzero(perm[:50] == m)[0][0]) + 1
        hits += p["top"][0]["feature"] == f"number {driver}"
    print(f"\nEXPLAIN forest planted drivers found: {hits} of 5")
    assert hits >= 3
    # error typing as the GBDT path: --top < 1 and a checkpoint whose F the data cannot provide exit 3
    assert cli.main(["explain", "--ckpt", ck, "--top", "0"] + data) == 3
    wide = str(tmp_path / "wide.npz")
    assert cli.main(["train", "--model", "rf", "--trees", "2", "--rf-max-depth", "2", "--lags", "3", "--ckpt", wide]
                    + data) == 0
    two = ["--data-source", "synthetic", "--n-draws", "2", "--seed", "4", "--device", "cpu"]
    assert cli.main(["explain", "--ckpt", wide] + two) == 3
    capsys.readouterr()
    assert cli.main(["explain", "--ckpt", wide, "--top", "1"] + data) == 0
    out = capsys.readouterr().out.strip().splitlines()
    assert "(lag " in out[0] and json.loads(out[-1])["explain"][0]["top"][0]["index"] < 186
