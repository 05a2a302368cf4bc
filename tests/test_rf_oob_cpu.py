"""Random forest out-of-bag evaluation and feature importances: the numpy specification
(euromillioner_amd/models/forest_oob.py) against the fp64 reference written from the definition
(tests/_rf_oob_ref.py), the comparison rules against mutations, persistence and the CLI.  No GPU."""
import json

import numpy as np
import pytest

import _rf_oob_ref as R
from euromillioner_amd.models import forest as FO
from euromillioner_amd.models import forest_oob as OOB
from euromillioner_amd.models.forest import RandomForest


def _data():
    R.build_case("d5")
    return R._cache["data", 1]


def _case(name):
    return R.build_case({"base": "d5", "few": "t3_d8", "range": "range7_12", "depth0": "d0"}[name])


@pytest.mark.parametrize("name", list(R.CASES))
def test_spec_matches_reference(name):
    rf, X, Y, rp, rc = R.build_case(name)
    proba, count = rf.oob_predict_proba(X)
    assert proba.dtype == np.float32 and proba.shape == (len(X), 62) and count.dtype == np.int32
    worst = R.check_oob(proba, count, rp, rc)
    print(f"{name}: worst error / budget {worst:.3f}, zero-count rows {int((rc == 0).sum())}")
    if name in ("d5", "t3_d8"):
        assert (rc == 0).any()  # the all-zero rule is exercised
    if name == "range7_12":
        assert rf.tree_start == 7 and rf.n_train == len(X)
    else:
        assert rf.tree_start == 0


def test_rules_reject_mutations():
    rf, X, Y, rp, rc = _case("range")
    proba, count = rf.oob_predict_proba(X)
    R.check_oob(proba, count, rp, rc)
    # the mean over ALL trees (predict_proba) with the right counts
    with pytest.raises(AssertionError):
        R.check_oob(np.where(rc[:, None] > 0, rf.predict_proba(X), 0).astype(np.float32), count, rp, rc)
    # local instead of global tree ids: the in-bag sets of trees 0..4, not 7..11
    rf.tree_start = 0
    try:
        mp, mc = rf.oob_predict_proba(X)
    finally:
        rf.tree_start = 7
    with pytest.raises(AssertionError):
        R.check_oob(mp, mc, rp, rc)
    # counts off by one
    with pytest.raises(AssertionError):
        R.check_oob(proba, count + 1, rp, rc)
    with pytest.raises(AssertionError):
        R.check_oob(proba, np.maximum(count - 1, 0), rp, rc)


def test_score_matches_reference_and_keys():
    rf, X, Y, rp, rc = _case("few")
    proba, count = rf.oob_predict_proba(X)
    tot = OOB.oob_totals_numpy(proba, count, Y)
    ref = R.metrics_reference(proba, count, Y)
    R.check_totals(tot, ref)
    score = rf.oob_score(X, Y)
    R.check_score(score, R.finish_reference(ref))
    assert score["rows"] + score["rows_without_oob_tree"] == len(X) and score["rows_without_oob_tree"] > 0
    assert 1 <= score["min_trees"] <= score["mean_trees"] <= 3


def test_score_ties_pick_the_earlier_index():
    n = 40
    proba = np.full((n, 62), 0.25, dtype=np.float32)
    first = np.uint64(sum(1 << j for j in (0, 1, 2, 3, 4, 50, 51)))
    tot = OOB.oob_totals_numpy(proba, np.ones(n, dtype=np.int32), np.full(n, first, dtype=np.uint64))
    assert tot["exact"] == n and tot["hits_main"] == 5 * n and tot["hits_star"] == 2 * n


def test_errors():
    rf, X, Y, _, _ = _case("base")
    with pytest.raises(ValueError):
        rf.oob_predict_proba(X[:-1])
    with pytest.raises(ValueError):
        rf.oob_score(X[:-1], Y[:-1])
    with pytest.raises(ValueError):
        RandomForest(device="cpu").oob_predict_proba(X)
    _, _, F = _data()
    nb = RandomForest(n_trees=2, max_depth=2, bootstrap=False, device="cpu").fit(X[:200], Y[:200], F)
    with pytest.raises(ValueError):
        nb.oob_predict_proba(X[:200])
    with pytest.raises(ValueError):
        rf.feature_importances("weight")


def test_save_load_keeps_oob_state(tmp_path):
    rf, X, Y, _, _ = _case("range")
    p = str(tmp_path / "rf.npz")
    rf.save(p)
    back = RandomForest.load(p)
    back.device = "cpu"
    assert back.n_train == len(X) and back.tree_start == 7
    a, b = rf.oob_predict_proba(X), back.oob_predict_proba(X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_old_format_file_loads(tmp_path):
    rf, X, Y, _, _ = _case("base")
    meta = {k: v for k, v in rf.meta().items() if k not in ("n_train", "tree_start")}
    p = str(tmp_path / "old.npz")
    np.savez(p, feat=rf.feat, value=rf.value, gain=rf.gain, cover=rf.cover,
             meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
    back = RandomForest.load(p)
    back.device = "cpu"
    assert back.n_train is None and back.tree_start == 0
    assert np.array_equal(back.oob_predict_proba(X)[0], rf.oob_predict_proba(X)[0])
    back.oob_predict_proba(X[:100])  # the row count is unknown, so it is not checked


def test_feature_importances_hand_example():
    """Output 0 equals feature 3 (no bootstrap, all features): the only split is on feature 3."""
    rng = np.random.default_rng(1)
    n = 400
    Xb = rng.integers(0, 2, size=(n, 62))
    Yb = np.zeros((n, 62), dtype=np.int64)
    Yb[:, 0] = Xb[:, 3]
    rf = RandomForest(n_trees=1, max_depth=1, feature_subset="all", bootstrap=False, device="cpu")
    rf.fit(FO.pack_bits(Xb), FO.pack_bits(Yb)[:, 0], 62)
    assert rf.feat[0, 0] == 3
    want = np.zeros(62)
    want[3] = 1.0
    for kind in ("gain", "cover", "splits"):
        imp = rf.feature_importances(kind)
        assert imp.dtype == np.float64 and imp.shape == (62,) and np.array_equal(imp, want), kind


def test_feature_importances_shares():
    rf, *_ = _case("base")
    split = rf.feat >= 0
    for kind, w in (("gain", rf.gain), ("cover", rf.cover), ("splits", np.ones(rf.feat.shape))):
        imp = rf.feature_importances(kind)
        assert abs(imp.sum() - 1.0) < 1e-12 and (imp >= 0).all()
        f = int(rf.feat[split][0])
        want = sum(float(w[t, nd]) for t, nd in zip(*np.nonzero(split)) if rf.feat[t, nd] == f)
        assert abs(imp[f] - want / float(np.asarray(w, dtype=np.float64)[split].sum())) < 1e-12
    rf0, *_ = _case("depth0")
    for kind in ("gain", "cover", "splits"):
        assert not rf0.feature_importances(kind).any()


def test_oob_is_a_held_out_estimate():
    """3000 draws, planted 0.7, 2000 rows fitted, 30 trees of depth 6: the out-of-bag hit rate lies below the
    resubstitution figure and nearer to the held-out one."""
    X, Y, F = _data()
    ntr = 2000
    rf = RandomForest(n_trees=30, max_depth=6, seed=2, device="cpu").fit(X[:ntr], Y[:ntr], F)
    oob = rf.oob_score(X[:ntr], Y[:ntr])["hits_main"]

    def hits(Xs, Ys):
        return OOB.oob_finish(OOB.oob_totals_numpy(rf.predict_proba(Xs), np.ones(len(Xs), dtype=np.int32), Ys))["hits_main"]

    resub, held = hits(X[:ntr], Y[:ntr]), hits(X[ntr:], Y[ntr:])
    print(f"oob {oob:.3f} resubstitution {resub:.3f} held-out {held:.3f}")
    assert oob < resub
    assert abs(oob - held) < abs(resub - held)


def _rf_line(capsys):
    out = capsys.readouterr().out
    recs = [json.loads(l) for l in out.splitlines() if l.startswith("{") and '"model": "rf"' in l]
    assert len(recs) == 1, out
    return recs[0]


def test_cli_oob_flag(capsys):
    from euromillioner_amd.cli import main

    base = ["train", "--model", "rf", "--device", "cpu", "--n-draws", "600", "--planted", "0.5", "--trees", "5",
            "--rf-max-depth", "4"]
    assert main(base) == 0
    plain = _rf_line(capsys)
    assert "oob" not in plain and "importances_top" not in plain
    assert main(base + ["--oob", "true"]) == 0
    rec = _rf_line(capsys)
    assert set(rec["oob"]) == set(R.SCORE_KEYS) and rec["oob"]["rows"] > 0
    top = rec["importances_top"]
    assert len(top) == 5 and all(0 <= f < 62 and 0 <= s <= 1 for f, s in top)
    assert [s for _, s in top] == sorted((s for _, s in top), reverse=True)
    assert {k: v for k, v in rec.items() if k not in ("oob", "importances_top", "seconds")} == \
        {k: v for k, v in plain.items() if k != "seconds"}
