"""The calibration specification (euromillioner_amd.calibration, numpy) against hand-worked rows and against the
independent fp64 reference tests/_calibration_ref.py, the comparison rules themselves against planted mistakes, and
``euromillioner evaluate --device cpu`` on a tiny checkpoint of each of the five model kinds.

Rules of the spec-vs-reference comparison (B = 1301 rows of ``R.draw_masks()``, every family of
``_fused_ref.FAMILIES``, both heads, the default edges):

* under bce x is the fp32 logit itself: the bins, counts and hits are equal, element by element, with no exception
  (the ``integers`` family puts a fifth of its logits exactly on logit(0.5) = 0, which is what tests ``>=``);
* under softmax the spec rounds x to fp32 before it compares: the bins are equal wherever the element is not
  ``near`` (|x - edge| < 1e-3 in fp64), and the totals are equal when no near element differs;
* sum_q and brier agree within 1e-9 relative.

The share of ``near`` elements under softmax is the slack the GPU test grants the kernel's fast exp / log, capped at
5 % per family (expected: 15 edges x 2e-3 x density, about 1 %); the measured shares are printed.  Under bce the GPU
test grants no slack, so the share is printed only.
"""
import json
import math

import numpy as np
import pytest

import _calibration_ref as CR
import _fused_ref as R

NEAR_CAP = CR.NEAR_CAP
HEADS = ("softmax", "bce")


def _cal():
    from euromillioner_amd import calibration as CAL

    return CAL


def _mask(mains, stars) -> int:
    m = 0
    for n in mains:
        m |= 1 << (n - 1)
    for s in stars:
        m |= 1 << (49 + s)
    return m


# ----------------------------------------------------------------------------------------------- hand case
def _hand_rows():
    """Three rows.  Row 0: every logit 0, draw 1 2 3 4 5 * 1 2.  Row 1: +2 on the drawn outputs of the same draw, -2
    elsewhere.  Row 2: every logit -0.5, draw 6 7 8 9 10 * 3 4.  The pads carry NaN: they are never read."""
    z = np.full((3, 64), np.nan, dtype=np.float32)
    tm = np.array([_mask(range(1, 6), (1, 2)), _mask(range(1, 6), (1, 2)), _mask(range(6, 11), (3, 4))], dtype=np.int64)
    z[0, :62] = 0.0
    z[1, :62] = -2.0
    z[1, [0, 1, 2, 3, 4, 50, 51]] = 2.0
    z[2, :62] = -0.5
    return z, tm


def _expect(cells: dict, brier) -> dict:
    out = {"counts": np.zeros((2, 16), dtype=np.int64), "hits": np.zeros((2, 16), dtype=np.int64),
           "sum_q": np.zeros((2, 16)), "brier": np.asarray(brier, dtype=np.float64)}
    for (g, b), (c, h, sq) in cells.items():
        out["counts"][g, b], out["hits"][g, b], out["sum_q"][g, b] = c, h, sq
    return out


def _same(got, want, rel=1e-12):
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["hits"], want["hits"]), (got["hits"], want["hits"])
    np.testing.assert_allclose(got["sum_q"], want["sum_q"], rtol=rel, atol=0)
    np.testing.assert_allclose(got["brier"], want["brier"], rtol=rel, atol=0)


def test_hand_case_bce():
    """Edges 0.25, 0.5, 0.75 -> x edges -ln 3, 0, ln 3 (1.0986).
    Row 0: x = 0 >= -ln 3 and >= 0, not >= ln 3 -> bin 2 for all 62; q = 1/2.  main: 50 elements, 5 hits, sum_q 25,
      brier 50 x 1/4; stars: 12 elements, 2 hits, sum_q 6, brier 12 x 1/4.
    Row 1: s = sigmoid(2) = 0.8808; x = 2 >= ln 3 -> bin 3 for the 5 + 2 drawn (all hits, q = s); x = -2 < -ln 3 ->
      bin 0 for the 45 + 10 others (q = 1 - s).  Every element misses its target by 1 - s: brier 50 (1 - s)^2 and
      12 (1 - s)^2.
    Row 2: u = sigmoid(-0.5) = 0.3775; -ln 3 <= -0.5 < 0 -> bin 1 for all; hits 5 and 2; brier 45 u^2 + 5 (1 - u)^2
      and 10 u^2 + 2 (1 - u)^2."""
    CAL = _cal()
    z, tm = _hand_rows()
    s, u = 1 / (1 + math.exp(-2.0)), 1 / (1 + math.exp(0.5))
    want = _expect({(0, 2): (50, 5, 25.0), (1, 2): (12, 2, 6.0),
                    (0, 3): (5, 5, 5 * s), (0, 0): (45, 0, 45 * (1 - s)), (1, 3): (2, 2, 2 * s), (1, 0): (10, 0, 10 * (1 - s)),
                    (0, 1): (50, 5, 50 * u), (1, 1): (12, 2, 12 * u)},
                   [12.5 + 50 * (1 - s) ** 2 + 45 * u * u + 5 * (1 - u) ** 2,
                    3.0 + 12 * (1 - s) ** 2 + 10 * u * u + 2 * (1 - u) ** 2])
    _same(CAL.calibration_np(z, tm, "bce", (0.25, 0.5, 0.75)), want)
    ref = CR.reference(z, _bits(tm), "bce", CAL.edges_x((0.25, 0.5, 0.75), "bce"))
    _same(ref, want)


def test_hand_case_softmax():
    """Edges 0.01, 0.05, 0.5 -> x edges ln 0.01 = -4.605, ln 0.05 = -2.996, ln 0.5 = -0.693.
    Rows 0 and 2 (constant logits: the same probabilities): main q = 1/50, x = -3.912 -> bin 1; stars q = 1/12,
      x = -2.485 -> bin 2.  Per row: main 50 elements, 5 hits, sum_q 1, brier 5 (1/50 - 1/5)^2 + 45 / 2500 = 0.18;
      stars 12 elements, 2 hits, sum_q 1, brier 2 (1/12 - 1/2)^2 + 10 / 144 = 5/12.
    Row 1: main D = 5 e^2 + 45 e^-2 = 43.035; drawn q = e^2 / D = 0.1717 (x = -1.762 -> bin 2), others
      q = e^-2 / D = 0.00314 (x = -5.762 -> bin 0); stars D = 2 e^2 + 10 e^-2 = 16.131; drawn q = 0.4581 (x = -0.781 ->
      bin 2), others q = 0.00839 (x = -4.781 -> bin 0).  brier 5 (qd - 1/5)^2 + 45 qo^2 and 2 (qd - 1/2)^2 + 10 qo^2."""
    CAL = _cal()
    z, tm = _hand_rows()
    e2, em2 = math.exp(2.0), math.exp(-2.0)
    dm, dst = 5 * e2 + 45 * em2, 2 * e2 + 10 * em2
    qd_m, qo_m, qd_s, qo_s = e2 / dm, em2 / dm, e2 / dst, em2 / dst
    want = _expect({(0, 1): (100, 10, 2.0), (1, 2): (24 + 2, 4 + 2, 2.0 + 2 * qd_s),
                    (0, 2): (5, 5, 5 * qd_m), (0, 0): (45, 0, 45 * qo_m), (1, 0): (10, 0, 10 * qo_s)},
                   [2 * 0.18 + 5 * (qd_m - 0.2) ** 2 + 45 * qo_m ** 2,
                    2 * (5 / 12) + 2 * (qd_s - 0.5) ** 2 + 10 * qo_s ** 2])
    _same(CAL.calibration_np(z, tm, "softmax", (0.01, 0.05, 0.5)), want, rel=1e-11)
    ref = CR.reference(z, _bits(tm), "softmax", CAL.edges_x((0.01, 0.05, 0.5), "softmax"))
    _same(ref, want, rel=1e-11)


def _bits(tm) -> np.ndarray:
    return ((np.asarray(tm, dtype=np.int64)[:, None] >> np.arange(62)) & 1).astype(np.int64)


# ----------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("loss", HEADS)
def test_edge_table_is_the_float32_rounding_of_the_definition(loss):
    CAL = _cal()
    ex = CAL.edges_x(CAL.DEFAULT_EDGES, loss)
    assert ex.dtype == np.float32 and ex.shape == (15,) and np.all(np.diff(ex) > 0)
    want = np.asarray(CR.edges_x_ref(CAL.DEFAULT_EDGES, loss))
    # equal up to one float32 step (two fp64 formulas of the same logarithm may round apart)
    assert np.all(np.abs(ex.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)))
    if loss == "bce":
        assert ex[CAL.DEFAULT_EDGES.index(0.5)] == 0.0


# ----------------------------------------------------------------------------------------------- spec vs reference
def _compare(CAL, family, loss, calibration_np=None, bins_np=None):
    """The comparison of the module docstring on one family and head; returns (near share, differing elements)."""
    z, Y, tm, _ = CR.case(family)
    ex = CAL.edges_x(CAL.DEFAULT_EDGES, loss)
    ref = CR.case_reference(family, loss, tuple(ex.tolist()))
    got = (calibration_np or CAL.calibration_np)(z.numpy(), tm, loss, CAL.DEFAULT_EDGES)
    bins = (bins_np or CAL.bins_np)(z.numpy(), loss, CAL.DEFAULT_EDGES).astype(np.int64)[:, :62]
    diff = bins != ref["bins"]
    if loss == "bce":
        assert not diff.any(), f"{family} bce: {int(diff.sum())} bins differ"
    else:
        assert not (diff & ~ref["near"]).any(), f"{family} softmax: a bin differs away from every edge"
        assert np.all(np.abs(bins - ref["bins"])[diff] == 1)
    if not diff.any():
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["hits"], ref["hits"])
        np.testing.assert_allclose(got["sum_q"], ref["sum_q"], rtol=1e-9, atol=0)
    else:  # a near element may sit one cell across: compare per group
        assert np.array_equal(got["counts"].sum(1), ref["counts"].sum(1))
        assert np.array_equal(got["hits"].sum(1), ref["hits"].sum(1))
        assert np.abs(got["counts"] - ref["counts"]).sum() <= 2 * int(diff.sum())
    np.testing.assert_allclose(got["sum_q"].sum(1), ref["sum_q"].sum(1), rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["brier"], ref["brier"], rtol=1e-9, atol=0)
    # the totals are the histogram of the spec's own bins
    own = CR.totals_from_bins(bins, Y.numpy())
    assert np.array_equal(got["counts"], own["counts"]) and np.array_equal(got["hits"], own["hits"])
    return float(ref["near"].mean()), int(diff.sum())


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("loss", HEADS)
def test_spec_matches_reference(loss, family):
    share, ndiff = _compare(_cal(), family, loss)
    print(f"{family} {loss}: near share {share:.4%}, {ndiff} bins differ")
    if loss == "softmax":  # the slack of the GPU test; bce gets none
        assert share <= NEAR_CAP, (family, share)


def test_invariants_and_single_bin():
    CAL = _cal()
    z, Y, tm, _ = CR.case("randn3")
    B = len(tm)
    for loss in HEADS:
        for edges in (CAL.DEFAULT_EDGES, (), (0.5,)):
            t = CAL.calibration_np(z.numpy(), tm, loss, edges)
            assert t["counts"].sum(1).tolist() == [50 * B, 12 * B]
            assert t["hits"].sum(1).tolist() == [5 * B, 2 * B]
            assert np.all(t["counts"][:, len(edges) + 1:] == 0)
            assert np.all(t["hits"] <= t["counts"])
        one = CAL.calibration_np(z.numpy(), tm, loss, ())
        assert one["counts"][:, 0].tolist() == [50 * B, 12 * B] and one["hits"][:, 0].tolist() == [5 * B, 2 * B]
        rep = CAL.report(one, B, loss, ())
        for g, k in (("main", 5), ("stars", 2)):
            row = rep[g]["bins"][0]
            assert row["count"] == rep[g]["count"] and rep[g]["bins"][1]["count"] == 0
            obs = rep[g]["hits"] / rep[g]["count"] / (k if loss == "softmax" else 1)
            assert row["observed"] == pytest.approx(obs, rel=1e-12)
            assert rep[g]["ece"] == pytest.approx(abs(row["mean_q"] - obs), rel=1e-9)
            assert rep[g]["brier"] == pytest.approx(one["brier"][GROUP[g]] / B, rel=1e-12)
        if loss == "softmax":  # each group's probabilities sum to 1 per row
            assert one["sum_q"][:, 0] == pytest.approx([B, B], rel=1e-9)


GROUP = {"main": 0, "stars": 1}


def test_report_ece_by_hand():
    CAL = _cal()
    tot = {"counts": np.zeros((2, 16), dtype=np.int64), "hits": np.zeros((2, 16), dtype=np.int64),
           "sum_q": np.zeros((2, 16)), "brier": np.array([3.0, 1.0])}
    tot["counts"][0, :2], tot["hits"][0, :2], tot["sum_q"][0, :2] = (60, 40), (6, 20), (3.0, 10.0)
    tot["counts"][1, 0], tot["hits"][1, 0], tot["sum_q"][1, 0] = 24, 4, 2.0
    rep = CAL.report(tot, 2, "bce")
    # main: bin 0 mean_q 0.05 vs 0.1, bin 1 mean_q 0.25 vs 0.5 -> ece 0.6 x 0.05 + 0.4 x 0.25 = 0.13
    assert rep["main"]["ece"] == pytest.approx(0.13) and rep["main"]["brier"] == 1.5
    assert rep["stars"]["ece"] == pytest.approx(abs(2 / 24 - 4 / 24))
    rep = CAL.report(tot, 2, "softmax")  # observed divided by k = 5: 0.02 and 0.1
    assert rep["main"]["ece"] == pytest.approx(0.6 * 0.03 + 0.4 * 0.15)
    assert rep["stars"]["bins"][0]["observed"] == pytest.approx(4 / 24 / 2)
    json.dumps(rep)


# ----------------------------------------------------------------------------------------------- planted mistakes
def _on_edge_logits(CAL):
    """bce logits placed exactly on the float32 edges: column o carries edge o % 15."""
    ex = CAL.edges_x(CAL.DEFAULT_EDGES, "bce")
    z = np.zeros((8, 64), dtype=np.float32)
    z[:, :62] = ex[np.arange(62) % 15][None, :]
    tm = R.draw_masks()[1:9].numpy().copy()
    return z, tm, ex


def _rejected(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_planted_mistakes_are_rejected(monkeypatch):
    """Each mistake is a mutation of the spec; the comparison that passes on the spec must fail on the mutant."""
    CAL = _cal()
    z3, tm3 = _hand_rows()
    z3 = np.nan_to_num(z3, nan=0.0)  # (the pads-counted mutant reads the pads)

    def spec_vs_ref(family="signal", loss="softmax"):
        _compare(CAL, family, loss)

    def hand():
        for loss in HEADS:
            ex = CAL.edges_x(CAL.DEFAULT_EDGES, loss)
            _same(CAL.calibration_np(z3, tm3, loss, CAL.DEFAULT_EDGES), CR.reference(z3, _bits(tm3), loss, ex), rel=1e-9)

    def invariants():
        t = CAL.calibration_np(z3, tm3, "bce", CAL.DEFAULT_EDGES)
        assert t["counts"].sum(1).tolist() == [150, 36] and t["hits"].sum(1).tolist() == [15, 6]

    def on_edge():
        z, tm, ex = _on_edge_logits(CAL)
        got = CAL.bins_np(z, "bce", CAL.DEFAULT_EDGES).astype(np.int64)
        assert np.array_equal(got, CR.reference(z, _bits(tm), "bce", ex)["bins"])
        assert np.array_equal(got[0], np.arange(62) % 15 + 1)  # x == edge k lies in bin k + 1

    for check in (spec_vs_ref, hand, invariants, on_edge):
        check()  # the spec itself passes every check

    with monkeypatch.context() as m:  # k swapped between the groups
        m.setattr(CAL, "K_NOMINAL", (2, 5))
        assert _rejected(spec_vs_ref) and _rejected(hand)
    with monkeypatch.context() as m:  # x > e instead of x >= e
        m.setattr(CAL, "_bin_of", lambda x, ex: (x.astype(np.float32)[..., None] > ex).sum(-1))
        assert _rejected(on_edge)
        assert _rejected(lambda: spec_vs_ref("integers", "bce"))  # a fifth of its logits sit on logit(0.5) = 0
    with monkeypatch.context() as m:  # the group boundary at 49 instead of 50
        m.setattr(CAL, "N_MAIN", 49)
        assert _rejected(spec_vs_ref) and _rejected(invariants)
    with monkeypatch.context() as m:  # pads 62-63 counted
        m.setattr(CAL, "NF", 64)
        assert _rejected(invariants) and _rejected(hand)
    with monkeypatch.context() as m:  # t = y under softmax
        m.setattr(CAL, "_target", lambda y, g, loss: y.astype(np.float64))
        assert _rejected(spec_vs_ref) and _rejected(hand)
    for check in (spec_vs_ref, hand, invariants, on_edge):
        check()  # and the spec is whole again


# ----------------------------------------------------------------------------------------------- argument errors
@pytest.mark.parametrize("edges", [(0.5, 0.5), (0.6, 0.5), (0.0, 0.5), (0.5, 1.0), (-0.1,), (1.5,), (float("nan"),),
                                   (float("inf"),), tuple(np.linspace(0.01, 0.99, 16)), ("a",), 0.5])
def test_bad_edges_raise(edges):
    CAL = _cal()
    z, tm = _hand_rows()
    for loss in HEADS:
        with pytest.raises(ValueError):
            CAL.calibration_np(z, tm, loss, edges)
        with pytest.raises(ValueError):
            CAL.edges_x(edges, loss)


def test_bad_arguments_raise():
    CAL = _cal()
    z, tm = _hand_rows()
    with pytest.raises(ValueError):
        CAL.calibration_np(z, tm, "hinge", CAL.DEFAULT_EDGES)
    with pytest.raises(ValueError):
        CAL.edges_x(CAL.DEFAULT_EDGES, "mse")
    with pytest.raises(ValueError):
        CAL.calibration_np(z[:, :61], tm, "bce")
    with pytest.raises(ValueError):
        CAL.calibration_np(z, tm[:2], "bce")
    with pytest.raises(ValueError):
        CAL.calibration_np(z, tm.astype(np.float64), "bce")
    with pytest.raises(ValueError):
        CAL.calibration_np(z[0], tm, "bce")
    with pytest.raises(ValueError):
        CAL.report(CAL.calibration_np(z, tm, "bce"), 0, "bce")
    with pytest.raises(ValueError):
        CAL.report(CAL.calibration_np(z, tm, "bce"), 3, "l2")
    # edges that are distinct in fp64 but collapse onto one float32 x
    with pytest.raises(ValueError):
        CAL.edges_x((0.5, 0.5 + 1e-12), "softmax")


# ----------------------------------------------------------------------------------------------- CLI
DATA = ["--n-draws", "400", "--planted", "0.6", "--seed", "3"]
TRAIN = {
    "mlp": (["--model", "mlp", "--steps", "6", "--batch", "64", "--eval-every", "0"], "m.zip", "softmax"),
    "mlp-bce": (["--model", "mlp", "--steps", "6", "--batch", "64", "--eval-every", "0", "--loss", "bce"], "b.zip", "bce"),
    "mlp-wide": (["--model", "mlp-wide", "--hidden", "32,16", "--steps", "4", "--batch", "64", "--eval-every", "0"],
                 "w.zip", "softmax"),
    "rf": (["--model", "rf", "--trees", "5", "--rf-max-depth", "4"], "f.npz", "bce"),
    "rf-lags": (["--model", "rf", "--trees", "4", "--rf-max-depth", "3", "--lags", "2"], "f2.npz", "bce"),
    "gbdt": (["--model", "gbdt", "--nround", "4"], "g.json", "bce"),
    "counts": (["--model", "counts", "--lags", "2"], "c.cnt", "softmax"),
}


def _result(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{") and '"calibration"' in l]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("kind", list(TRAIN))
def test_cli_evaluate_cpu(kind, tmp_path, capsys):
    from euromillioner_amd.cli import main

    flags, name, loss = TRAIN[kind]
    ck = str(tmp_path / name)
    extra = ["--workdir", str(tmp_path)] if kind == "gbdt" else []
    assert main(["train", "--device", "cpu", "--ckpt", ck] + flags + DATA + extra) == 0
    capsys.readouterr()
    lags = ["--lags", "2"] if kind in ("rf-lags",) else []
    assert main(["evaluate", "--device", "cpu", "--ckpt", ck] + DATA + lags) == 0
    out = capsys.readouterr().out
    res = _result(out)
    CR.check_result(res, loss, "numpy")
    assert res["model"] == {"mlp-bce": "mlp", "mlp-wide": "mlp", "rf-lags": "rf"}.get(kind, kind)
    n_lags = 2 if kind in ("rf-lags", "counts") else 1
    assert res["rows"] == (400 - n_lags) - int(0.7 * (400 - n_lags))
    # the printed table: one line per non-empty bin
    filled = sum(1 for g in ("main", "stars") for r in res["calibration"][g]["bins"] if r["count"])
    assert sum(1 for l in out.splitlines() if l.startswith("  [")) == filled
    # other edges, from the flag
    assert main(["evaluate", "--device", "cpu", "--ckpt", ck, "--edges", "0.1,0.5"] + DATA + lags) == 0
    CR.check_result(_result(capsys.readouterr().out), loss, "numpy", n_edges=2)


def test_cli_evaluate_refusals(tmp_path, capsys):
    from euromillioner_amd.cli import main

    assert main(["evaluate", "--ckpt", str(tmp_path / "nope.zip")] + DATA) == 3
    assert main(["evaluate"] + DATA) == 3
    ck = str(tmp_path / "ref.json")
    assert main(["train", "--model", "gbdt", "--device", "cpu", "--target", "reference", "--objective",
                 "reg:squarederror", "--eval-metric", "rmse", "--nround", "2", "--ckpt", ck, "--workdir",
                 str(tmp_path)] + DATA) == 0
    capsys.readouterr()
    assert main(["evaluate", "--device", "cpu", "--ckpt", ck] + DATA) == 3
    ck2 = str(tmp_path / "g.json")
    assert main(["train", "--model", "gbdt", "--device", "cpu", "--nround", "2", "--ckpt", ck2, "--workdir",
                 str(tmp_path)] + DATA) == 0
    assert main(["evaluate", "--device", "cpu", "--ckpt", ck2, "--edges", "0.5,0.4"] + DATA) == 3  # bad edges
    assert main(["evaluate", "--device", "cpu", "--ckpt", ck2, "--model", "rf"] + DATA) == 3  # not that kind
    capsys.readouterr()
    assert main(["evaluate", "--device", "cpu", "--ckpt", ck2, "--model", "gbdt"] + DATA) == 0
    assert _result(capsys.readouterr().out)["model"] == "gbdt"
    assert main(["evaluate", "--device", "cpu", "--ckpt", ck2, "--n-draws", "1"]) == 3  # empty validation split
    assert main(["evaluate", "--ckpt", ck2, "--data-source", "device", "--n-draws", "400"]) == 3
