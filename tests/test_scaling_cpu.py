"""The scaling specification (euromillioner_amd.scaling, numpy) against the independent fp64 reference
tests/_scaling_ref.py, the reference's own derivatives and budget, the comparisons against planted mistakes, the
Newton fit on planted parameters, the ``.cal`` file, and ``euromillioner calibrate`` / ``evaluate --calibrator`` on
``--device cpu``.

Rules:

* ``stats_np`` equals the reference within 1e-12 of ``A`` (fp64 rounding of a few ten thousand terms);
* the reference's gradients and Hessians equal central differences of its own ``L``.  The logits there are
  multiples of 2^-6 inside [-4, 4] and the points are dyadic, so ``u`` is exact in float32 and ``L`` is a smooth
  fp64 function; with step h = 2^-8 the truncation error of a central difference is h^2 / 6 (first) or h^2 / 12
  (second) times a derivative two orders up, which is at most (2 z_max)^2 = 64 times the magnitude sum of the
  statistic: the tolerance is ``64 h^2 A``;
* the kernel's formulas in honest numpy float32, in the kernel's summation order, stay within the budget ``K u A``
  (half of what the GPU test allows) on every input of the GPU test: the budget is reachable.
"""
import json
import os

import numpy as np
import pytest

import _scaling_ref as SR

HEADS = ("softmax", "bce")


def _sc():
    from euromillioner_amd import scaling as SC

    return SC


# ----------------------------------------------------------------------------------------------- spec vs reference
def _spec_stats(SC, z, masks, B, offset, loss, a, b):
    """The statistics the way every engine is addressed: rows [0, B), row s against masks[offset + s + 1]."""
    return SC.stats_np(z[:B], masks[offset + 1:offset + 1 + B], loss, a, b)


def _check_spec(stats=_spec_stats, B=513, offsets=(0, 17)):
    SC = _sc()
    z, m = SR.inputs()
    for loss in HEADS:
        for p, (a, b) in enumerate(SR.POINTS[loss]):
            for off in offsets:
                S, A = SR.case_reference(loss, p, B, off)
                got = stats(SC, z, m, B, off, loss, a, b)
                assert got.shape == (2, 6) and got.dtype == np.float64
                bad = ~(np.abs(got - S.sum(0)) <= 1e-12 * A.sum(0))
                assert not bad.any(), (loss, a, b, off, got[bad], S.sum(0)[bad])


def test_stats_np_matches_reference():
    _check_spec()
    _check_spec(B=1)
    SC = _sc()
    z, m = SR.inputs()
    for loss in HEADS:  # the rows of a group's zeros are exact zeros
        got = SC.stats_np(z, m[1:514], loss)
        assert (got[:, [2, 4, 5]] == 0).all() if loss == "softmax" else (got[:, 5] > 0).all()


def _smooth_case(rows=200):
    rng = np.random.default_rng(77)
    z = np.zeros((rows, 64), dtype=np.float32)
    z[:, :62] = np.clip(np.round(1.5 * rng.standard_normal((rows, 62)) * 64) / 64, -4, 4)
    return z, SR.bits(SR.masks(rows, seed=9))


@pytest.mark.parametrize("loss", HEADS)
def test_derivatives_are_central_differences_of_L(loss):
    z, Y = _smooth_case()
    h = 2.0 ** -8

    def L(a, b):
        return SR.reference(z, Y, loss, a, b)[0][:, 0]

    for a0, b0 in ((1.0, 0.0), (0.25, 0.0 if loss == "softmax" else 3.0), (4.0, 0.0 if loss == "softmax" else -3.0)):
        S, A = SR.reference(z, Y, loss, (a0, a0), (b0, b0))
        tol = 64 * h * h * A
        ap, am, bp, bm = (a0 + h,) * 2, (a0 - h,) * 2, (b0 + h,) * 2, (b0 - h,) * 2
        a_, b_ = (a0, a0), (b0, b0)
        fd = {1: (L(ap, b_) - L(am, b_)) / (2 * h), 3: (L(ap, b_) - 2 * L(a_, b_) + L(am, b_)) / (h * h)}
        if loss == "bce":
            fd[2] = (L(a_, bp) - L(a_, bm)) / (2 * h)
            fd[5] = (L(a_, bp) - 2 * L(a_, b_) + L(a_, bm)) / (h * h)
            fd[4] = (L(ap, bp) - L(ap, bm) - L(am, bp) + L(am, bm)) / (4 * h * h)
        for k, v in fd.items():
            assert np.all(np.abs(v - S[:, k]) <= tol[:, k]), (loss, a0, b0, SR.STATS[k], v, S[:, k], tol[:, k])
        if loss == "softmax":
            assert not S[:, [2, 4, 5]].any()
        assert np.all(S[:, 3] > 0) and (loss == "softmax" or np.all(S[:, 3] * S[:, 5] > S[:, 4] ** 2))  # convex


@pytest.mark.parametrize("loss", HEADS)
def test_L_at_identity_is_the_draw_metrics_loss(loss):
    from euromillioner_amd.metrics import draw_metrics

    SC = _sc()
    z, m = SR.inputs()
    tm = m[1:514]
    Y = SR.bits(tm)
    if loss == "softmax":  # (a group without a target bit adds its log-sum-exp here and 0 there: n_g is clamped, the
        keep = (Y[:, :50].sum(1) > 0) & (Y[:, 50:].sum(1) > 0)  # sum over no bits is not)
        assert 400 < keep.sum() < 513
        z, tm, Y = z[keep], tm[keep], Y[keep]
    rows = len(z)
    want = draw_metrics(z[:, :62].astype(np.float64), Y, loss)["loss"]
    assert SC.row_loss(SC.stats_np(z, tm, loss), rows, loss) == pytest.approx(want, rel=1e-12)
    S, _ = SR.reference(z, Y, loss)
    assert (S[0, 0] + S[1, 0]) / (rows if loss == "softmax" else 62 * rows) == pytest.approx(want, rel=1e-12)


@pytest.mark.parametrize("loss", HEADS)
def test_honest_float32_in_kernel_order_is_within_half_the_allowance(loss):
    z, m = SR.inputs()
    worst = 0.0
    for p, (a, b) in enumerate(SR.POINTS[loss]):
        for B in SR.BS:
            for off, seed in ((0, None), (17, None), (0, 2)):
                S, A = SR.case_reference(loss, p, B, off, seed)
                idx = SR.sample_index(B, seed).astype(np.int64) if seed is not None else off + np.arange(B)
                got = SR.kernel_order_f32(z[:B], SR.bits(m[idx + 1]), loss, a, b).astype(np.float64)
                assert got.shape == ((B + 255) // 256, 2, 6)
                Sb, Ab = SR.block_sums(S), SR.block_sums(A)
                assert SR.within(got, Sb, Ab, factor=SR.FACTOR / 2).all(), (loss, a, b, B, off, seed)
                assert SR.within(got.sum(0), S.sum(0), A.sum(0), factor=SR.FACTOR / 2).all(), (loss, a, b, B)
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst = max(worst, float(np.nanmax(np.abs(got - Sb) / SR.budget(Ab))))
    print(f"{loss}: honest float32 uses at most {worst:.4f} of the budget K u A")


# ----------------------------------------------------------------------------------------------- planted mistakes
def _rejected(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


def _check_apply(apply=None):
    SC = _sc()
    apply = apply or SC.apply_np
    z, _ = SR.inputs()
    for a, b in (((1.0, 1.0), (0.0, 0.0)), ((0.3, 1.7), (0.7, -0.1)), ((4.0, 0.25), (-3.0, 3.0))):
        got = apply(z[:65], a, b)
        assert got.dtype == np.float32 and got.shape == (65, 64) and not got[:, 62:].any()
        want = np.zeros((65, 64), dtype=np.float32)
        for s in range(65):
            for o in range(62):
                g = 0 if o < 50 else 1
                want[s, o] = np.float32(np.float32(np.float32(a[g]) * z[s, o]) + np.float32(b[g]))
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (a, b)


def test_apply_np_is_a_scalar_float32_loop():
    _check_apply()


def test_planted_mistakes_are_rejected(monkeypatch):
    """Each mistake is a mutation of the spec; the comparison that passes on the spec must fail on the mutant."""
    SC = _sc()
    _check_spec()
    _check_apply()
    for attr, val in (("N_MAIN", 49), ("N_MAIN", 51),  # the group boundary
                      ("NF", 64),  # the pad columns read (they hold NaN)
                      ("_group_n", lambda yg, g: np.full(len(yg), (5.0, 2.0)[g])),  # nominal k instead of n_g
                      ("_variance", lambda q, zg, ez: (q * zg * zg).sum(1))):  # an uncentred variance
        with monkeypatch.context() as mp:
            mp.setattr(SC, attr, val)
            assert _rejected(_check_spec), (attr, val)

    def swapped(SC, z, m, B, off, loss, a, b):  # g_a and g_b swapped
        return _spec_stats(SC, z, m, B, off, loss, a, b)[:, [0, 2, 1, 3, 4, 5]]

    def no_hab(SC, z, m, B, off, loss, a, b):  # h_ab dropped
        st = _spec_stats(SC, z, m, B, off, loss, a, b)
        st[:, 4] = 0.0
        return st

    def one_more(SC, z, m, B, off, loss, a, b):  # a row past B counted
        return _spec_stats(SC, z, m, B + 1, off, loss, a, b)

    def this_draw(SC, z, m, B, off, loss, a, b):  # masks[idx] instead of masks[idx + 1]
        return _spec_stats(SC, z, m, B, off - 1, loss, a, b)

    for mutant in (swapped, no_hab, this_draw):
        assert _rejected(lambda: _check_spec(mutant)), mutant.__name__
    assert _rejected(lambda: _check_spec(one_more, B=257)), "one_more"

    def fused(z, a, b):  # an fma in apply: one rounding instead of two
        out = np.zeros((len(z), 64), dtype=np.float32)
        for g, sl in enumerate((slice(0, 50), slice(50, 62))):
            out[:, sl] = (float(np.float32(a[g])) * z[:, sl].astype(np.float64) + float(np.float32(b[g]))).astype(np.float32)
        return out

    assert _rejected(lambda: _check_apply(fused))
    _check_spec()  # and the spec is whole again
    _check_apply()


# ----------------------------------------------------------------------------------------------- the fit
PLANTED = {"softmax": (2.0, 0.0), "bce": (2.0, -1.0)}


@pytest.mark.parametrize("loss", HEADS)
def test_fit_np_recovers_planted_parameters(loss):
    SC = _sc()
    ta, tb = PLANTED[loss]
    z, tm = SR.planted(loss, a=ta, b=tb)
    fit = SC.fit_np(z, tm, loss)
    assert fit["a"].dtype == np.float32 and fit["b"].dtype == np.float32
    assert all(fit["converged"]) and max(fit["iterations"]) <= 30, fit
    assert np.all(fit["L_after"] <= fit["L_before"])
    if loss == "softmax":
        assert not fit["b"].any()
    S, _ = SR.reference(z, SR.bits(tm), loss, fit["a"], fit["b"])
    dist = [SR.distance(fit["a"][g], fit["b"][g], ta, tb, S[g]) for g in (0, 1)]
    print(f"{loss}: a {fit['a'].tolist()} b {fit['b'].tolist()} after {fit['iterations']} iterations, "
          f"{fit['passes']} passes; standardised distance {dist}")
    assert max(dist) <= 5.0, dist
    assert np.allclose(S[:, 0], fit["L_after"], rtol=1e-12)
    # the gradient vanishes as far as one float32 ulp of the parameters can tell
    ulp = np.spacing(np.maximum(np.abs(fit["a"]), np.abs(fit["b"]))).astype(np.float64)
    assert np.all(np.abs(S[:, 1]) <= 2 * (S[:, 3] + np.abs(S[:, 4])) * ulp), (S, ulp)
    assert np.all(np.abs(S[:, 2]) <= 2 * (np.abs(S[:, 4]) + S[:, 5]) * ulp), (S, ulp)


@pytest.mark.parametrize("loss", HEADS)
def test_fit_np_leaves_calibrated_data_alone(loss):
    SC = _sc()
    z, tm = SR.planted(loss, seed=5, a=1.0, b=0.0)
    fit = SC.fit_np(z, tm, loss)
    S, _ = SR.reference(z, SR.bits(tm), loss, fit["a"], fit["b"])
    assert all(fit["converged"])
    assert max(SR.distance(fit["a"][g], fit["b"][g], 1.0, 0.0, S[g]) for g in (0, 1)) <= 5.0


def test_fit_argument_errors():
    SC = _sc()
    z, tm = SR.planted("bce", rows=8)
    for bad in (lambda: SC.fit_np(z, tm, "hinge"), lambda: SC.fit_np(z[:, :61], tm, "bce"),
                lambda: SC.fit_np(z, tm[:3], "bce"), lambda: SC.fit_np(z[:0], tm[:0], "bce"),
                lambda: SC.stats_np(z, tm, "bce", (0.0, 1.0)), lambda: SC.stats_np(z, tm, "bce", (1.0, -1.0)),
                lambda: SC.stats_np(z, tm, "bce", (1.0, float("nan"))), lambda: SC.stats_np(z, tm, "bce", (1.0, float("inf"))),
                lambda: SC.stats_np(z, tm, "bce", (1.0, 1.0), (0.0, float("nan"))),
                lambda: SC.stats_np(z, tm, "softmax", (1.0, 1.0), (0.0, 0.5)), lambda: SC.stats_np(z, tm, "bce", (1.0,)),
                lambda: SC.apply_np(z, (1.0, 0.0), (0.0, 0.0)), lambda: SC.apply_np(z[:, :60], (1.0, 1.0), (0.0, 0.0)),
                lambda: SC.stats_np(z, tm.astype(np.float64), "bce")):
        with pytest.raises(ValueError):
            bad()


# ----------------------------------------------------------------------------------------------- the .cal file
def _calibrator(SC, loss="bce"):
    a = np.array([1.2345678, 0.1], dtype=np.float32)
    b = np.array([-0.3333333, 1e-7], dtype=np.float32) if loss == "bce" else np.zeros(2, dtype=np.float32)
    return SC.Calibrator(loss, a, b, {"model": "mlp", "lags": 1, "first": 279, "last": 339, "rows": 60,
                                      "iterations": [5, 6], "converged": [True, True], "loss_before": 3.5,
                                      "loss_after": 3.25, "checkpoint": "m.zip"})


@pytest.mark.parametrize("loss", HEADS)
def test_cal_file_round_trips_bit_for_bit(loss, tmp_path):
    SC = _sc()
    cal = _calibrator(SC, loss)
    path = str(tmp_path / "m.cal")
    cal.save(path)
    back = SC.Calibrator.load(path)
    assert back.loss == loss and back.record == cal.record
    assert np.array_equal(back.a.view(np.int32), cal.a.view(np.int32))
    assert np.array_equal(back.b.view(np.int32), cal.b.view(np.int32))
    d = json.load(open(path))
    assert d["a"] == [float(v) for v in cal.a] and d["a_hex"] == [float(v).hex() for v in cal.a]
    assert d["checkpoint"] == "m.zip" and d["first"] == 279 and d["last"] == 339 and d["version"] == 1


def test_malformed_cal_files_are_refused(tmp_path):
    SC = _sc()
    good = _calibrator(SC).to_dict()
    path = str(tmp_path / "bad.cal")
    one = float(1).hex()
    mutations = [{"version": 2}, {"version": None}, {"loss": "hinge"}, {"loss": None}, {"a_hex": [one]},
                 {"a_hex": [one, "zz"]}, {"a_hex": [one, float(0).hex()]}, {"a_hex": [one, float(-1).hex()]},
                 {"a_hex": [one, "inf"]}, {"a_hex": [one, "nan"]}, {"b_hex": [one, "nan"]}, {"b_hex": [one, "-inf"]},
                 {"a_hex": [1.0, 1.0]}, {"a_hex": None}, {"b_hex": "0x0p+0"}, {"a_hex": [one, (1.0 + 2.0 ** -40).hex()]},
                 {"last": -1}, {"rows": "many"}, {"loss": "softmax"}]  # (softmax with a shift)
    for mut in mutations:
        with open(path, "w") as f:
            json.dump({**good, **mut}, f)
        with pytest.raises(ValueError):
            SC.Calibrator.load(path)
    for text in ("", "not json", "[1, 2]", "{"):
        with open(path, "w") as f:
            f.write(text)
        with pytest.raises(ValueError):
            SC.Calibrator.load(path)
    with open(path, "w") as f:
        json.dump(good, f)
    SC.Calibrator.load(path)
    with pytest.raises(ValueError):
        SC.Calibrator("bce", (1.0, float("inf")), (0.0, 0.0))


# ----------------------------------------------------------------------------------------------- CLI
DATA = ["--n-draws", "400", "--planted", "0.6", "--seed", "3"]
TRAIN = {
    "mlp": (["--model", "mlp", "--steps", "6", "--batch", "64", "--eval-every", "0"], "m.zip", "softmax", 1),
    "counts": (["--model", "counts", "--lags", "2"], "c.cnt", "softmax", 2),
    "rf": (["--model", "rf", "--trees", "5", "--rf-max-depth", "4"], "f.npz", "bce", 1),
    "gbdt": (["--model", "gbdt", "--nround", "4"], "g.json", "bce", 1),
}


def _result(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{") and '"calibration"' in l]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def _train(kind, tmp_path, capsys) -> str:
    from euromillioner_amd.cli import main

    flags, name, _, _ = TRAIN[kind]
    ck = str(tmp_path / name)
    extra = ["--workdir", str(tmp_path)] if kind == "gbdt" else []
    assert main(["train", "--device", "cpu", "--ckpt", ck] + flags + DATA + extra) == 0
    capsys.readouterr()
    return ck


@pytest.mark.parametrize("kind", list(TRAIN))
def test_cli_calibrate_then_evaluate_cpu(kind, tmp_path, capsys):
    from euromillioner_amd.cli import main

    SC = _sc()
    _, _, loss, lags = TRAIN[kind]
    ck = _train(kind, tmp_path, capsys)
    n = 400 - lags
    margin = int(0.7 * n)
    last = margin + (n - margin) // 2
    assert main(["calibrate", "--device", "cpu", "--ckpt", ck] + DATA) == 0
    out = capsys.readouterr().out
    res = _result(out)
    assert res["model"] == kind and res["engine"] == "numpy" and res["loss"] == loss
    assert res["fit_rows"] == last - margin and res["rows"] == n - last and res["out"] == ck + ".cal"
    for part in ("before", "after"):
        assert res[part]["val"]["count"] == n - last and res[part]["calibration"]["rows"] == n - last
    c = res["calibrator"]
    assert (c["model"], c["lags"], c["first"], c["last"], c["rows"]) == (kind, lags, margin, last, last - margin)
    assert c["checkpoint"] == os.path.basename(ck) and c["loss"] == loss
    assert c["loss_after"] <= c["loss_before"] and max(c["iterations"]) <= 30
    assert out.count("  before ") == 2 and out.count("  after ") == 2
    cal = SC.Calibrator.load(ck + ".cal")
    assert cal.to_dict() == c and np.all(cal.a > 0) and (loss == "bce" or not cal.b.any())
    # evaluate through it: the rows after the fit range, the report of calibrate's "after"
    assert main(["evaluate", "--device", "cpu", "--ckpt", ck, "--calibrator", ck + ".cal"] + DATA) == 0
    out = capsys.readouterr().out
    ev = _result(out)
    assert f"samples [{last}, {n}) through {os.path.basename(ck)}.cal" in out.splitlines()[0]
    assert ev["rows"] == n - last and ev["first"] == last and ev["calibrator"] == c
    assert ev["val"] == res["after"]["val"] and ev["calibration"] == res["after"]["calibration"]
    # other places and shares
    other = str(tmp_path / "other.cal")
    assert main(["calibrate", "--device", "cpu", "--ckpt", ck, "--out", other, "--fit-pct", "0.25", "--fit-rows", "20"] + DATA) == 0
    res2 = _result(capsys.readouterr().out)
    assert res2["fit_rows"] == 20 and res2["calibrator"]["last"] == margin + 20 and os.path.exists(other)


def test_cli_evaluate_without_a_calibrator_is_unchanged(tmp_path, capsys):
    """``evaluate`` against a direct call of the engine it wrapped before the set-up moved into a helper."""
    from euromillioner_amd import calibration as CAL
    from euromillioner_amd import config as C
    from euromillioner_amd import train as T
    from euromillioner_amd.data.draws import mask_bits
    from euromillioner_amd.models.count_table import CountTable
    from euromillioner_amd.pipeline import load_draws

    ck = _train("counts", tmp_path, capsys)
    cfg = C.build_config(None, {"data.n_draws": 400, "data.planted": 0.6, "data.seed": 3, "device": "cpu",
                                "ckpt.path": ck})
    res = T.evaluate(cfg)
    out = capsys.readouterr().out
    host = mask_bits(load_draws(cfg).numbers).view(np.int64)
    ct = CountTable.load(ck, "cpu")
    n = 400 - ct.lags
    margin = int(0.7 * n)
    want = T._evaluate_numpy(lambda c0, c1: ct.logits_np(host, np.arange(c0, c1)), host[ct.lags:], margin, n,
                             "softmax", CAL.DEFAULT_EDGES)
    assert set(res) == {"checkpoint", "engine", "model", "lags", "loss", "rows", "val", "calibration", "edges"}
    assert res["val"] == want["val"] and res["calibration"] == want["calibration"] and res["rows"] == n - margin
    assert out.splitlines()[0] == f"{n - margin} validation rows, counts (softmax head, numpy)"


def test_cli_calibrate_refusals(tmp_path, capsys, monkeypatch):
    from euromillioner_amd.cli import main

    SC = _sc()
    assert main(["calibrate", "--ckpt", str(tmp_path / "nope.zip")] + DATA) == 3
    assert main(["calibrate"] + DATA) == 3
    ck = _train("counts", tmp_path, capsys)
    cpu = ["--device", "cpu", "--ckpt", ck]
    assert main(["calibrate", "--model", "rf"] + cpu + DATA) == 3  # not that kind
    for pct in ("0", "1", "-0.5", "1e-9", "nan"):  # a share outside (0, 1), or one that leaves the fit without rows
        assert main(["calibrate", "--fit-pct", pct] + cpu + DATA) == 3, pct
    assert main(["calibrate", "--fit-rows", "0"] + cpu + DATA) == 3
    assert main(["calibrate", "--fit-pct", "half"] + cpu + DATA) == 2  # not a number: a configuration error
    assert main(["calibrate"] + cpu + ["--n-draws", "1"]) == 3  # empty validation split
    assert not os.path.exists(ck + ".cal")
    with monkeypatch.context() as mp:
        mp.setenv("WORLD_SIZE", "2")
        assert main(["calibrate"] + cpu + DATA) == 3
    assert main(["calibrate"] + cpu + DATA) == 0
    # evaluate --calibrator
    assert main(["evaluate", "--calibrator", str(tmp_path / "nope.cal")] + cpu + DATA) == 3
    bad = str(tmp_path / "bad.cal")
    cal = SC.Calibrator.load(ck + ".cal")
    for rec in ({"model": "mlp"}, {"lags": 1}, {"last": 398}, {"last": 100}, {"last": None}):
        SC.Calibrator(cal.loss, cal.a, cal.b, {**cal.record, **rec}).save(bad)
        assert main(["evaluate", "--calibrator", bad] + cpu + DATA) == 3, rec
    with open(bad, "w") as f:
        f.write("{}")
    assert main(["evaluate", "--calibrator", bad] + cpu + DATA) == 3
    ck2 = _train("rf", tmp_path, capsys)  # a bce checkpoint against the softmax calibrator
    assert main(["evaluate", "--device", "cpu", "--ckpt", ck2, "--calibrator", ck + ".cal"] + DATA) == 3
    capsys.readouterr()
    assert main(["evaluate", "--calibrator", ck + ".cal"] + cpu + DATA) == 0
