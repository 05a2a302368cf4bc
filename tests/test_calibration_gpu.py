"""em_draw_calibration (csrc/calibration.hip) and what is built on it, against the fp64 reference
tests/_calibration_ref.py fed the SAME fp32 logits.

Cases per family of ``_fused_ref.FAMILIES`` and head: B in (1, 255, 256, 257, 1301) x offset in (0, 17), once through
a sample index with repeats, once with a row stride of 72; the logits' pads 62-63 hold NaN.  Rules:

* per-element bins (``want_bins``): under bce equal to the reference's, exactly (float32 against the same table);
  under softmax an element may differ only where it is ``near`` (|x - edge| < 1e-3 in fp64, the project's margin for
  the same fast exp / log), only by one bin, and at most 5 % of the elements of a family may (the cap that
  tests/test_calibration_cpu.py holds the reference's near share to); pads come back 0;
* the ``counts`` / ``hits`` totals are exactly the histogram of the device's own bins against the target bits;
* ``sum_q`` per cell and ``brier`` per group agree with the reference within ``_fused_ref.LOSS_TOL`` relative (plus
  2^-126 per element of ``sum_q``: fp32 holds no smaller q, and a randn80 cell can consist of such elements alone);
  where a softmax element sits one cell across, ``sum_q`` is compared summed over the bins of each group;
* outputs sit between poisoned guard rows that must come back unchanged, refusals leave the outputs untouched, and
  two calls give bit-equal partials.
"""
import json

import numpy as np
import pytest
import torch

import _calibration_ref as CR
import _fused_ref as R

pytestmark = pytest.mark.gpu

HEADS = ("softmax", "bce")
# (B, offset, sidx seed, row stride)
CASES = [(B, off, None, 64) for B in (1, 255, 256, 257, 1301) for off in (0, 17)] + [(1301, 0, 2, 64), (1301, 17, None, 72)]
POISON_I, POISON_F, POISON_B = -123456789, -7.5, 0xAB


@pytest.fixture(scope="module")
def draws():
    return R.draw_masks().cuda()


def _device_logits(z: torch.Tensor, ld: int) -> torch.Tensor:
    """The case's logits on the device with NaN pads, as a [B, 64] view of rows ``ld`` floats apart."""
    buf = torch.full((z.shape[0], ld), float("nan"), dtype=torch.float32)
    buf[:, :62] = z[:, :62]
    return buf.cuda()[:, :64]


def _guarded(B: int, want_bins: bool = True):
    """Poisoned buffers with one guard row before and after the outputs; returns (buffers, out views)."""
    from euromillioner_amd.ops import calibration as OC

    nb = OC.calibration_blocks(B)
    big = {"counts": torch.full((nb + 2, 2, 16), POISON_I, dtype=torch.int32, device="cuda"),
           "hits": torch.full((nb + 2, 2, 16), POISON_I, dtype=torch.int32, device="cuda"),
           "sum_q": torch.full((nb + 2, 2, 16), POISON_F, dtype=torch.float32, device="cuda"),
           "brier": torch.full((nb + 2, 2), POISON_F, dtype=torch.float32, device="cuda")}
    if want_bins:
        big["bins"] = torch.full((B + 2, 64), POISON_B, dtype=torch.uint8, device="cuda")
    return big, {k: v[1:-1] for k, v in big.items()}


def _guards_intact(big: dict) -> None:
    for k, v in big.items():
        poison = POISON_F if v.dtype == torch.float32 else POISON_B if v.dtype == torch.uint8 else POISON_I
        assert bool((v[0] == poison).all()) and bool((v[-1] == poison).all()), f"guard row of {k} written"


def _untouched(big: dict) -> None:
    torch.cuda.synchronize()
    for k, v in big.items():
        poison = POISON_F if v.dtype == torch.float32 else POISON_B if v.dtype == torch.uint8 else POISON_I
        assert bool((v == poison).all()), f"{k} written by a refused call"


FLT_MIN = 2.0 ** -126  # a predicted value below the smallest normal fp32 may reach the device sum as 0


def _rel_close(got, ref, what, n=0):
    """|got - ref| <= LOSS_TOL |ref| + n FLT_MIN; ``n``: the elements summed (fp32 cannot hold a q below FLT_MIN, the
    fp64 reference can: randn80 under softmax has such elements)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = ~(np.abs(got - ref) <= R.LOSS_TOL * np.abs(ref) + np.asarray(n, dtype=np.float64) * FLT_MIN)
    assert not bad.any(), (what, got[bad], ref[bad])


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("loss", HEADS)
def test_calibration_matches_reference(draws, loss, family):
    from euromillioner_amd import calibration as CAL
    from euromillioner_amd.ops import calibration as OC

    ex = CAL.edges_x(CAL.DEFAULT_EDGES, loss)
    differ = elements = near = 0
    for B, off, seed, ld in CASES:
        what = f"{family} {loss} B={B} offset={off} sidx={seed} ld={ld}"
        z, Y, _, sidx = CR.case(family, B, off, seed)
        ref = CR.case_reference(family, loss, tuple(ex.tolist()), B, off, seed)
        lg = _device_logits(z, ld)
        assert lg.stride(0) == ld
        big, out = _guarded(B)
        kw = dict(offset=0, sidx=sidx.cuda()) if sidx is not None else dict(offset=off)
        parts = OC.draw_calibration(lg, draws, B, loss, want_bins=True, out=out, **kw)
        again = OC.draw_calibration(lg, draws, B, loss, want_bins=True, **kw)
        torch.cuda.synchronize()
        _guards_intact(big)
        assert parts["counts"].shape == (OC.calibration_blocks(B), 2, 16) == ((B + 255) // 256, 2, 16)
        for k in ("counts", "hits", "bins"):
            assert torch.equal(parts[k], again[k]), (what, k)
        for k in ("sum_q", "brier"):  # bit for bit
            assert torch.equal(parts[k].view(torch.int32), again[k].view(torch.int32)), (what, k)
        # without bins: the same partials
        plain = OC.draw_calibration(lg, draws, B, loss, **kw)
        assert "bins" not in plain
        for k in ("counts", "hits"):
            assert torch.equal(parts[k], plain[k]), (what, k)
        for k in ("sum_q", "brier"):
            assert torch.equal(parts[k].view(torch.int32), plain[k].view(torch.int32)), (what, k)
        # bins, element by element
        bins = parts["bins"].cpu().numpy().astype(np.int64)
        assert not bins[:, 62:].any(), what
        diff = bins[:, :62] != ref["bins"]
        if loss == "bce":
            assert not diff.any(), f"{what}: {int(diff.sum())} bins differ"
        else:
            assert not (diff & ~ref["near"]).any(), f"{what}: a bin differs away from every edge"
            assert np.all(np.abs(bins[:, :62] - ref["bins"])[diff] == 1), what
        differ += int(diff.sum())
        near += int(ref["near"].sum())
        elements += diff.size
        # integers: the histogram of the device's own bins, and the invariants
        tot = OC.sum_calibration(parts)
        own = CR.totals_from_bins(bins, Y.numpy())
        assert np.array_equal(tot["counts"], own["counts"]) and np.array_equal(tot["hits"], own["hits"]), what
        assert tot["counts"].dtype == np.int64 and tot["sum_q"].dtype == np.float64
        assert tot["counts"].sum(1).tolist() == [50 * B, 12 * B] and tot["hits"].sum(1).tolist() == [5 * B, 2 * B]
        assert int(parts["counts"].min()) >= 0 and int(parts["hits"].min()) >= 0
        # float sums
        if not diff.any():
            assert np.array_equal(tot["counts"], ref["counts"]) and np.array_equal(tot["hits"], ref["hits"]), what
            _rel_close(tot["sum_q"], ref["sum_q"], what + " sum_q", ref["counts"])
        _rel_close(tot["sum_q"].sum(1), ref["sum_q"].sum(1), what + " sum_q per group", ref["counts"].sum(1))
        _rel_close(tot["brier"], ref["brier"], what + " brier")
    print(f"{family} {loss}: {differ} of {elements} bins differ from the fp64 reference, {near} are near an edge")
    if loss == "softmax":  # (differing bins are near ones: at most the share the CPU test caps)
        assert differ <= near <= CR.NEAR_CAP * elements


def test_fewer_edges_and_none(draws):
    """n_edges 0, 1 and 3: the unused tail of the edge table must not count."""
    from euromillioner_amd import calibration as CAL
    from euromillioner_amd.ops import calibration as OC

    B = 257
    z, Y, _, _ = CR.case("signal", B, 0, None)
    lg = _device_logits(z, 64)
    for loss in HEADS:
        for edges in ((), (0.5,), (0.02, 0.2, 0.9)):
            ref = CR.reference(z.numpy(), Y.numpy(), loss, CAL.edges_x(edges, loss))
            parts = OC.draw_calibration(lg, draws, B, loss, edges=edges, want_bins=True)
            bins = parts["bins"].cpu().numpy().astype(np.int64)[:, :62]
            assert bins.max() <= len(edges)
            diff = bins != ref["bins"]
            assert not (diff & ~ref["near"]).any() and (loss == "softmax" or not diff.any())
            tot = OC.sum_calibration(parts)
            assert not tot["counts"][:, len(edges) + 1:].any()
            assert tot["counts"].sum(1).tolist() == [50 * B, 12 * B]
            _rel_close(tot["brier"], ref["brier"], f"{loss} {edges} brier")


def test_refusals_leave_outputs_untouched(draws):
    from euromillioner_amd import calibration as CAL
    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.ops import calibration as OC

    B = 300
    z, _, _, _ = CR.case("randn3", 1301, 0, None)
    lg = _device_logits(z[:B], 64).contiguous()
    big, out = _guarded(B)
    n = draws.shape[0]
    sidx = torch.arange(B, dtype=torch.int32, device="cuda")
    bad_calls = [
        dict(loss="hinge"), dict(edges=(0.5, 0.4)), dict(edges=(0.0, 0.5)), dict(edges=tuple(np.linspace(0.01, 0.99, 16))),
        dict(edges=(float("nan"),)), dict(B=0), dict(B=-1), dict(B=B + 1), dict(offset=-1), dict(offset=n - B),
        dict(logits=lg.cpu()), dict(logits=lg.double()), dict(logits=lg[:, :62]), dict(logits=lg.view(-1)[:B * 32].view(B, 32)),
        dict(logits=torch.zeros(B, 66, device="cuda")[:, :64]), dict(logits=torch.zeros(B * 64 + 4, device="cuda")[1:B * 64 + 1].view(B, 64)),
        dict(masks=draws.cpu()), dict(masks=draws.int()), dict(sidx=sidx.long()), dict(sidx=sidx[:B - 1]),
        dict(sidx=sidx + (n - B)), dict(sidx=sidx - 1), dict(sidx=sidx.cpu()),
    ]
    for kw in bad_calls:
        args = dict(logits=lg, masks=draws, B=B, loss="bce", edges=CAL.DEFAULT_EDGES, offset=0, sidx=None)
        args.update(kw)
        with pytest.raises(ValueError):
            OC.draw_calibration(args["logits"], args["masks"], args["B"], args["loss"], edges=args["edges"],
                                offset=args["offset"], sidx=args["sidx"], want_bins=True, out=out)
    with pytest.raises(ValueError):  # an output of the wrong shape
        OC.draw_calibration(lg, draws, B, "bce", want_bins=True, out={**out, "counts": out["counts"][:1]})
    _untouched(big)

    # raw calls: EM_ERR_ARG before any launch
    import ctypes

    ex = CAL.edges_x(CAL.DEFAULT_EDGES, "bce")
    ebuf = (ctypes.c_float * 15)(*[float(v) for v in ex])
    eptr = ctypes.cast(ebuf, ctypes.c_void_p)
    good = [lg.data_ptr(), 64, draws.data_ptr(), None, B, 0, 1, eptr, 15, out["counts"].data_ptr(),
            out["hits"].data_ptr(), out["sum_q"].data_ptr(), out["brier"].data_ptr(), out["bins"].data_ptr(),
            N.stream_handle(lg.device)]
    raw_bad = [(0, None), (2, None), (7, None), (9, None), (10, None), (11, None), (12, None),  # null pointers
               (8, 16), (8, -1), (1, 60), (1, 66), (1, 63), (4, 0), (4, -5), (4, 2 ** 31 - 1), (4, 2 ** 40), (5, -1),
               (0, lg.data_ptr() + 4), (6, 2), (6, -1)]
    for pos, val in raw_bad:
        a = list(good)
        a[pos] = val
        with pytest.raises(ValueError):
            N.call("em_draw_calibration", *a)
    _untouched(big)
    assert OC.calibration_blocks(0) == 0 and OC.calibration_blocks(256) == 1 and OC.calibration_blocks(257) == 2
    # and the good call does write
    N.call("em_draw_calibration", *good)
    torch.cuda.synchronize()
    _guards_intact(big)
    assert int(out["counts"].sum()) == 62 * B


def _models(draws):
    from euromillioner_amd.models.count_table import CountTable
    from euromillioner_amd.models.mlp import FusedSmallMLP

    yield "fused-softmax", FusedSmallMLP(loss="softmax", state_dict=R.make_state("biased")), "softmax", None
    yield "fused-bce", FusedSmallMLP(loss="bce", state_dict=R.make_state("biased")), "bce", None
    ct = CountTable(2, 1.0, "cuda").fit_draw_masks(draws, 0, 4000)
    yield "counts-lags2", ct, "softmax", ct._tmasks(draws)


def test_calibrate_model_chunks(draws):
    """B = 1301 from offset 5 in chunks of 100 and in one chunk: identical integers, ``val`` as ``evaluate``."""
    from euromillioner_amd import calibration as CAL
    from euromillioner_amd.ops import calibration as OC

    B, off = 1301, 5
    for name, model, loss, tgt in _models(draws):
        runs = {c: OC.calibrate_model(model, draws, B, loss, CAL.DEFAULT_EDGES, offset=off, chunk=c, target_masks=tgt)
                for c in (100, 1 << 20)}
        ident = torch.arange(off, off + B, dtype=torch.int32, device="cuda")
        runs["sidx"] = OC.calibrate_model(model, draws, B, loss, CAL.DEFAULT_EDGES, sidx=ident, chunk=500,
                                          target_masks=tgt)
        base = runs[1 << 20]
        for c, r in runs.items():
            ev = model.evaluate(draws, B, offset=off, chunk=c if isinstance(c, int) else 500)
            assert r["val"]["count"] == ev["count"] == B
            for k, v in ev.items():
                assert r["val"][k] == pytest.approx(v, rel=1e-9, abs=1e-12), (name, c, k)
            for g, width, kk in (("main", 50, 5), ("stars", 12, 2)):
                a, b = r["calibration"][g], base["calibration"][g]
                assert [x["count"] for x in a["bins"]] == [x["count"] for x in b["bins"]], (name, c, g)
                assert [x["observed"] for x in a["bins"]] == [x["observed"] for x in b["bins"]], (name, c, g)
                assert a["count"] == width * B and a["hits"] == kk * B
                assert a["brier"] == pytest.approx(b["brier"], rel=1e-6) and a["ece"] == pytest.approx(b["ece"], rel=1e-5, abs=1e-9)
        # against the specification fed the model's own logits
        z = model.logits(draws, B, offset=off).cpu().numpy()
        tm = (draws if tgt is None else tgt)[off + 1:off + 1 + B].cpu().numpy()
        spec = CAL.report(CAL.calibration_np(z, tm, loss, CAL.DEFAULT_EDGES), B, loss, CAL.DEFAULT_EDGES)
        for g in ("main", "stars"):
            moved = sum(abs(x["count"] - y["count"]) for x, y in zip(base["calibration"][g]["bins"], spec[g]["bins"]))
            assert moved <= 2 * CR.NEAR_CAP * spec[g]["count"] and (loss == "softmax" or moved == 0), (name, g, moved)
            assert base["calibration"][g]["brier"] == pytest.approx(spec[g]["brier"], rel=R.LOSS_TOL)
        json.dumps(base)
    with pytest.raises(ValueError):
        OC.calibrate_model(model, draws, 0, loss)
    with pytest.raises(ValueError):
        OC.calibrate_model(model, draws, B, loss, chunk=0)


def _spec_report(z: torch.Tensor, tm: torch.Tensor, edges):
    from euromillioner_amd import calibration as CAL

    return CAL.report(CAL.calibration_np(z.cpu().numpy(), tm.cpu().numpy(), "bce", edges), len(tm), "bce", edges)


def _same_report(res: dict, spec: dict) -> None:
    for g in ("main", "stars"):
        a, b = res["calibration"][g], spec[g]
        assert [x["count"] for x in a["bins"]] == [x["count"] for x in b["bins"]], g  # bce: the bins are exact
        assert [x["observed"] for x in a["bins"]] == [x["observed"] for x in b["bins"]], g
        for x, y in zip(a["bins"], b["bins"]):
            if x["count"]:
                assert x["mean_q"] == pytest.approx(y["mean_q"], rel=R.LOSS_TOL)
        assert a["brier"] == pytest.approx(b["brier"], rel=R.LOSS_TOL)


def _result(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{") and '"calibration"' in l]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_cli_evaluate_tree_checkpoints_on_the_gpu(tmp_path, capsys):
    """A small forest .npz (2 lags) and a small GBDT .json over the 62 draw bits, both trained here: ``evaluate``
    reports engine hip, and its calibration is the specification's on the device logits copied to the host."""
    from euromillioner_amd import calibration as CAL
    from euromillioner_amd.cli import main
    from euromillioner_amd.data.csv_io import write_draws_csv
    from euromillioner_amd.data.draws import DrawSet, positional_split
    from euromillioner_amd.models.forest import RandomForest
    from euromillioner_amd.models.gbdt import GBDT
    from euromillioner_amd.models.mlp import FusedSmallMLP
    from euromillioner_amd.ops import tree_inputs as TI

    ds = DrawSet.synthetic(n=700, seed=4, planted=0.6, calendar=False)  # no dates: the GBDT reads the 62 bits only
    csv = str(tmp_path / "draws.csv")
    write_draws_csv(csv, ds)
    data = ["--data-source", "csv", "--data-path", csv]
    masks = FusedSmallMLP.prepare(ds.numbers)

    ck = str(tmp_path / "f.npz")
    assert main(["train", "--model", "rf", "--trees", "6", "--rf-max-depth", "4", "--lags", "2", "--ckpt", ck] + data) == 0
    capsys.readouterr()
    assert main(["evaluate", "--ckpt", ck] + data) == 0
    res = _result(capsys.readouterr().out)
    CR.check_result(res, "bce", "hip")
    n = len(ds) - 2
    margin = positional_split(n, 70.0)
    assert res["model"] == "rf" and res["rows"] == n - margin
    rf = RandomForest.load(ck)
    X, Y, _ = TI.rf_rows(masks, 2, first=margin, count=n - margin)
    _same_report(res, _spec_report(rf.predict_proba_device(X, out_logit=True), Y, CAL.DEFAULT_EDGES))

    ck = str(tmp_path / "g.json")
    assert main(["train", "--model", "gbdt", "--nround", "4", "--ckpt", ck, "--workdir", str(tmp_path)] + data) == 0
    capsys.readouterr()
    assert main(["evaluate", "--ckpt", ck, "--edges", "0.05,0.1,0.2,0.5"] + data) == 0
    res = _result(capsys.readouterr().out)
    CR.check_result(res, "bce", "hip", n_edges=4)
    n = len(ds) - 1
    margin = positional_split(n, 70.0)
    assert res["model"] == "gbdt" and res["features"] == 62 and res["rows"] == n - margin
    g = GBDT.load(ck)
    z = g.predict_margin_draw_masks(masks, (margin, n))
    _same_report(res, _spec_report(z, masks[margin + 1:n + 1], (0.05, 0.1, 0.2, 0.5)))
