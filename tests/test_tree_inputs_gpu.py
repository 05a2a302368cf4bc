"""Tree-model inputs from device draw masks (csrc/tree_inputs.hip) and the forest / GBDT trained from them.

Every comparison is exact equality against a path the suite already trusts: the host specification of the
packed lag rows (tests/_tree_inputs_spec.py, tied to ``draw_features`` by tests/test_tree_inputs_cpu.py), numpy
bit counts, ``apply_bins(multi_hot)``, and ``RandomForest.fit`` / ``GBDT.fit`` (HIP backend) on host matrices
built from the same masks copied back."""
import numpy as np
import pytest

from _tree_inputs_spec import lag_rows_spec, random_masks, unpack

pytestmark = pytest.mark.gpu

BLOCK = 256  # samples per block of em_rf_lag_rows


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def rand_masks():
    """(host int64 [n], device copy), n past two blocks of every kernel here."""
    m = random_masks(2 * BLOCK + 40, 7)
    return m, _dev(m)


# ----------------------------------------------------------------------------- lag rows
@pytest.mark.parametrize("lags", [1, 2, 3, 4])
def test_lag_rows_equal_the_specification(rand_masks, lags):
    import torch

    from euromillioner_amd.ops import tree_inputs as TI

    m, d = rand_masks
    n = len(m)
    # one sample on lags + 1 draws; both sides of one block and one past it; first > 0 ending at the last draw
    windows = [(d[:lags + 1], m[:lags + 1], 0, None), (d, m, 0, BLOCK - 1), (d, m, 0, BLOCK), (d, m, 0, BLOCK + 1),
               (d, m, 5, None), (d, m, n - lags - 1, 1)]
    for dm, hm, first, count in windows:
        X, Y, F = TI.rf_rows(dm, lags, first=first, count=count)
        S = len(hm) - lags - first if count is None else count
        Xs, Ys = lag_rows_spec(hm, lags, first, S)
        assert F == 62 * lags and X.dtype == torch.int64 and Y.dtype == torch.int64
        assert tuple(X.shape) == (S, (F + 63) // 64) and tuple(Y.shape) == (S,)
        assert np.array_equal(X.cpu().numpy().view(np.uint64), Xs), (lags, first, count)
        assert np.array_equal(Y.cpu().numpy().view(np.uint64), Ys), (lags, first, count)
        used = F - 64 * (X.shape[1] - 1)  # bits of the last word that carry features
        if used < 64:
            assert not (X.cpu().numpy().view(np.uint64)[:, -1] >> np.uint64(used)).any()
    assert (m.view(np.uint64) >> np.uint64(62)).any()  # (the inputs carried bits 62-63)


# ----------------------------------------------------------------------------- bit counts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100003])
def test_bit_counts_equal_numpy(n):
    from euromillioner_amd.ops import tree_inputs as TI

    m = random_masks(n, n)
    d = _dev(m)
    bits = (m.view(np.uint64)[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    got = TI.bit_counts(d, 0, n)
    assert got.dtype == np.int64 and got.shape == (64,)
    assert np.array_equal(got, bits.sum(0).astype(np.int64))
    a, b = n // 3, n - n // 5  # a sub-window (empty for n = 1)
    assert np.array_equal(TI.bit_counts(d, a, b), bits[a:b].sum(0).astype(np.int64))


# ----------------------------------------------------------------------------- GBDT inputs
@pytest.mark.parametrize("S", [1, 3, 1023, 1025])
def test_gbdt_inputs_equal_apply_bins(S):
    import torch

    from euromillioner_amd.models.gbdt import apply_bins
    from euromillioner_amd.ops import tree_inputs as TI

    first = 2
    m = random_masks(first + S + 1, 100 + S)
    d = _dev(m)
    X = unpack(m[first:first + S]).astype(np.float64)
    Yref = unpack(m[first + 1:first + S + 1]).astype(np.float32)
    g = np.random.default_rng(S)
    for varied in ((1 << 62) - 1, 0, int(g.integers(0, 1 << 62))):
        cuts = [np.array([0.5]) if (varied >> f) & 1 else np.zeros(0) for f in range(62)]
        bins, Y = TI.gbdt_draw_inputs(d, first, S, varied)
        assert bins.dtype == torch.uint8 and Y.dtype == torch.float32 and bins.shape == Y.shape == (S, 62)
        assert np.array_equal(bins.cpu().numpy(), apply_bins(X, cuts)), (S, hex(varied))
        assert np.array_equal(Y.cpu().numpy(), Yref), (S, hex(varied))
    only, none = TI.gbdt_draw_inputs(d, first, S + 1, (1 << 62) - 1, targets=False)  # up to the last draw
    assert none is None and np.array_equal(only.cpu().numpy(), unpack(m[first:]).astype(np.uint8))


def test_gbdt_inputs_past_2_31_elements():
    """35M rows: the flat element index passes 2^31 (62 * 35M = 2.17e9), where a 32-bit offset would wrap.  The
    last rows against the specification, the first rows too (a wrapped store would land there), and both
    outputs' sums against the bit counts of torch's own shifts."""
    import torch

    from euromillioner_amd.data.device_gen import generate_masks
    from euromillioner_amd.ops import tree_inputs as TI

    S = 35_000_000
    assert S * 62 > 2 ** 31
    d = generate_masks(S + 1, seed=2, planted=0.5)
    varied = (1 << 62) - 1 - (1 << 9)
    bins, Y = TI.gbdt_draw_inputs(d, 0, S, varied)
    for a, b in ((S - 500, S), (0, 500)):
        m = d[a:b + 1].cpu().numpy()
        want = unpack(m[:-1])
        want[:, 9] = 0
        assert np.array_equal(bins[a:b].cpu().numpy(), want.astype(np.uint8))
        assert np.array_equal(Y[a:b].cpu().numpy(), unpack(m[1:]).astype(np.float32))
    ones = sum(int(((d[:S] >> j) & 1).sum()) for j in range(62) if j != 9)
    assert int(bins.sum(dtype=torch.int64)) == ones
    assert int(Y.sum(dtype=torch.float64)) == sum(int(((d[1:] >> j) & 1).sum()) for j in range(62))
    counts = TI.bit_counts(d, 0, S)
    assert int(counts[:62].sum()) - int(counts[9]) == ones and not counts[62:].any()
    del bins, Y, d
    torch.cuda.empty_cache()  # (11 GB: not kept cached under the rest of the suite)


# ----------------------------------------------------------------------------- refusals
def test_argument_errors_raise_before_any_write(rand_masks):
    import torch

    from euromillioner_amd.ops import tree_inputs as TI

    m, d = rand_masks
    n = len(m)
    S, lags = 16, 2
    X = torch.full((S, 2), 0x5A5A, dtype=torch.int64, device="cuda")
    Y = torch.full((S,), 0x5A5A, dtype=torch.int64, device="cuda")
    bins = torch.full((S, 62), 0x5A, dtype=torch.uint8, device="cuda")
    T = torch.full((S, 62), 7.0, dtype=torch.float32, device="cuda")
    bad_masks = [torch.from_numpy(m), d.to(torch.int32), d[::2], d.view(-1, 2)[:, 0]]
    for bm in bad_masks:
        with pytest.raises(ValueError):
            TI.rf_rows(bm, lags, 0, S, out=(X, Y))
        with pytest.raises(ValueError):
            TI.gbdt_draw_inputs(bm, 0, S, (1 << 62) - 1, out=(bins, T))
        with pytest.raises(ValueError):
            TI.bit_counts(bm, 0, 4)
    for bad_lags in (0, 5, -1):
        with pytest.raises(ValueError):
            TI.rf_rows(d, bad_lags, 0, S, out=(X, Y))
    for first, count in ((0, 0), (0, -3), (-1, S), (n - lags - S + 1, S), (n, 1)):  # S < 1, windows past the end
        with pytest.raises(ValueError):
            TI.rf_rows(d, lags, first, count, out=(X, Y))
    for first, count in ((0, 0), (-1, S), (n - S, S), (n, 1)):
        with pytest.raises(ValueError):
            TI.gbdt_draw_inputs(d, first, count, (1 << 62) - 1, out=(bins, T))
    with pytest.raises(ValueError):
        TI.rf_rows(d[:lags], lags)  # count=None with no sample at all
    for a, b in ((-1, 3), (5, 4), (0, n + 1)):
        with pytest.raises(ValueError):
            TI.bit_counts(d, a, b)
    with pytest.raises(ValueError):  # outputs of the wrong shape / dtype are refused too
        TI.rf_rows(d, lags, 0, S, out=(X[:, :1], Y))
    with pytest.raises(ValueError):
        TI.gbdt_draw_inputs(d, 0, S, 0, out=(bins, T.double()))
    torch.cuda.synchronize()
    assert bool((X == 0x5A5A).all()) and bool((Y == 0x5A5A).all())
    assert bool((bins == 0x5A).all()) and bool((T == 7.0).all())
    X2, Y2, _ = TI.rf_rows(d, lags, 0, S, out=(X, Y))  # and the same buffers are filled by a valid call
    Xs, Ys = lag_rows_spec(m, lags, 0, S)
    assert X2 is X and np.array_equal(X.cpu().numpy().view(np.uint64), Xs) and np.array_equal(Y.cpu().numpy().view(np.uint64), Ys)


# ----------------------------------------------------------------------------- forest fit
@pytest.fixture(scope="module")
def planted_masks():
    from euromillioner_amd.data.device_gen import generate_masks

    d = generate_masks(3000, seed=11, planted=0.9)
    return d.cpu().numpy(), d


@pytest.mark.parametrize("lags", [1, 2])
def test_forest_fit_from_masks_equals_host_fit(planted_masks, lags, tmp_path):
    from euromillioner_amd.models.forest import RandomForest

    m, d = planted_masks
    n = len(m) - lags
    for a, b in ((0, n), (700, 2500)):
        dev = RandomForest(8, 5, seed=3, device="cuda").fit_draw_masks(d, lags=lags, rows=(a, b))
        Xh, Yh = lag_rows_spec(m, lags, a, b - a)
        host = RandomForest(8, 5, seed=3, device="cuda").fit(Xh, Yh, 62 * lags)
        assert host.backend_used == dev.backend_used == "hip"
        assert (dev.F, dev.k, dev.n_train, dev.tree_start) == (host.F, host.k, host.n_train, host.tree_start)
        for name in ("feat", "value", "gain", "cover"):
            x, y = getattr(dev, name), getattr(host, name)
            assert x.dtype == y.dtype and np.array_equal(x, y), (lags, a, b, name)
        assert (dev.feat >= 0).sum() > 8  # (the planted structure does grow trees)
    path = str(tmp_path / f"rf{lags}.npz")
    dev.save(path)
    back = RandomForest.load(path)
    Xv, _ = lag_rows_spec(m, lags, 0, 400)
    assert back.meta() == dev.meta()
    assert np.array_equal(back.predict_proba(Xv), dev.predict_proba(Xv))
    assert np.array_equal(back.apply(Xv, backend="hip"), dev.apply(Xv, backend="numpy"))
    with pytest.raises(ValueError):
        RandomForest(2, 2).fit_draw_masks(d, lags=lags, group=object())


# ----------------------------------------------------------------------------- GBDT fit
@pytest.fixture(scope="module")
def gbdt_case():
    """2000 generated draws with bit 5 cleared everywhere (a constant column: an empty cut), and the host
    matrices of the next-draw task built from the masks copied back."""
    from euromillioner_amd.data.device_gen import generate_masks

    d = generate_masks(2000, seed=5, planted=0.9)
    d &= ~(1 << 5)
    m = d.cpu().numpy()
    return m, d, unpack(m[:-1]).astype(np.float64), unpack(m[1:]).astype(np.float64)


@pytest.mark.parametrize("subsample", [1.0, 0.7])
def test_gbdt_fit_from_masks_equals_host_fit(gbdt_case, subsample):
    from euromillioner_amd.models.gbdt import GBDT

    m, d, X, Y = gbdt_case
    n, a = len(m) - 1, 1400
    kw = dict(eta=0.5, max_depth=3, nround=4, gamma=0.0, subsample=subsample, seed=9, backend="hip")
    host = GBDT(**kw).fit(X[:a], Y[:a], evals={"train": (X[:a], Y[:a]), "test": (X[a:], Y[a:])})
    dev = GBDT(**kw).fit_draw_masks(d, (0, a), evals={"train": (0, a), "test": (a, n)})
    assert dev.backend_used == "hip" and dev.num_feature == 62 and dev.n_tasks == 62
    assert len(dev.cuts) == 62 and len(dev.cuts[5]) == 0
    for c, h in zip(dev.cuts, host.cuts):
        assert c.dtype == h.dtype and np.array_equal(c, h)
    for name in ("status", "feat", "sbin", "leaf", "gain", "cover", "split_value"):
        x, y = getattr(dev.trees, name), getattr(host.trees, name)
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    assert (dev.trees.status == 1).sum() > 62  # (trees were grown)
    assert dev.history == host.history and len(dev.history) == 4 and set(dev.history[0]) == {"round", "train", "test"}
    assert dev.train_history == host.train_history and len(dev.train_history) == 4
    assert dev.to_json() == host.to_json()
    for r0, r1 in ((a, n), (0, 257), (n - 1, n)):
        got = dev.predict_margin_draw_masks(d, (r0, r1))
        want = host.predict_margin(X[r0:r1]).astype(np.float32)
        assert tuple(got.shape) == (r1 - r0, 64)
        g = got.cpu().numpy()
        assert np.array_equal(g[:, :62].view(np.int32), want.view(np.int32)) and not g[:, 62:].any()
    assert np.array_equal(dev.predict(X[a:]), host.predict(X[a:]))  # (host rows through the device-fitted model)


def test_gbdt_fit_from_masks_refusals(gbdt_case):
    from euromillioner_amd.models.gbdt import GBDT

    m, d, X, Y = gbdt_case
    n = len(m) - 1
    with pytest.raises(ValueError):
        GBDT(nround=1, backend="hip").fit_draw_masks(d, (0, 100), group=object())
    with pytest.raises(ValueError):
        GBDT(nround=1, backend="hip", objective="multi:softprob").fit_draw_masks(d, (0, 100))
    with pytest.raises(ValueError):
        GBDT(nround=1, backend="hip").fit_draw_masks(d, (0, n + 1))  # draw n + 1 does not exist
    with pytest.raises(ValueError):
        GBDT(nround=1, backend="hip").fit_draw_masks(d, (0, 100), evals={"test": (100, n + 1)})
    sq = GBDT(nround=2, max_depth=2, objective="reg:squarederror", eval_metric="rmse", backend="hip")
    sq.fit_draw_masks(d, (0, 500), evals={"test": (500, 800)})
    ref = GBDT(nround=2, max_depth=2, objective="reg:squarederror", eval_metric="rmse", backend="hip")
    ref.fit(X[:500], Y[:500], evals={"test": (X[500:800], Y[500:800])})
    assert sq.history == ref.history and np.array_equal(sq.trees.leaf, ref.trees.leaf)


# ----------------------------------------------------------------------------- end to end
def _cfg(model, tmp_path, **over):
    from euromillioner_amd import config as C

    base = {"model": model, "data.source": "device", "data.n_draws": 20001, "data.planted": 0.9, "data.seed": 4,
            "log.level": "WARNING"}
    base.update(over)
    return C.build_config(None, base)


def _finish(part):
    from euromillioner_amd.ops import fused_mlp as FM

    tot = part.double().sum(0).cpu().numpy()
    res = {k: float(tot[i] / max(tot[7], 1.0)) for i, k in enumerate(FM.METRIC_NAMES[:-1])}
    res["count"] = int(tot[7])
    return res


def _aligned(val, logits, targets):
    """The integer-valued metrics against the numpy definition on explicit target rows: equal as the suite's
    draw-metric tests establish (tests/test_draw_metrics_gpu.py), and off for targets shifted by a draw."""
    from euromillioner_amd import metrics as M

    ref = M.draw_metrics(logits[:, :62].cpu().numpy(), targets, loss="bce")
    for k in ("hits_main", "hits_star", "exact", "count"):
        assert val[k] == ref[k], (k, val[k], ref[k])


def test_train_rf_on_device_draws(tmp_path):
    from euromillioner_amd.data.device_gen import generate_masks
    from euromillioner_amd.models.forest import RandomForest
    from euromillioner_amd.ops import fused_mlp as FM
    from euromillioner_amd.train import train

    path = str(tmp_path / "rf.npz")
    res = train(_cfg("rf", tmp_path, **{"rf.n_trees": 8, "rf.oob": True, "ckpt.path": path}))
    n, margin = 20000, 14000
    assert (res["model"], res["backend"], res["world"], res["trees"]) == ("rf", "hip", 1, 8)
    assert res["train_samples"] == margin and res["val_samples"] == n - margin and res["checkpoint"] == path
    d = generate_masks(20001, seed=4, planted=0.9)
    m = d.cpu().numpy()
    rf = RandomForest.load(path)
    assert rf.n_train == margin and rf.F == 62
    Xh, Yh = lag_rows_spec(m, 1, 0, n)
    lg = rf.predict_proba_device(Xh[margin:], out_logit=True)
    assert res["val"] == _finish(FM.draw_metrics(lg, d, n - margin, loss="bce", offset=margin))
    _aligned(res["val"], lg, unpack(m[margin + 1:n + 1]))
    rf.device = "cuda"
    assert res["oob"] == rf.oob_score(Xh[:margin], Yh[:margin])
    imp = rf.feature_importances("gain")
    assert res["importances_top"] == [[int(f), float(imp[f])] for f in np.argsort(-imp, kind="stable")[:5]]


def test_train_gbdt_on_device_draws(tmp_path, capsys):
    import torch

    from euromillioner_amd.data.device_gen import generate_masks
    from euromillioner_amd.models.gbdt import GBDT
    from euromillioner_amd.ops import fused_mlp as FM
    from euromillioner_amd.train import train

    path = str(tmp_path / "gbdt.json")
    res = train(_cfg("gbdt", tmp_path, **{"gbdt.nround": 3, "ckpt.path": path}))
    n, margin = 20000, 14000
    assert res["pipeline"] == "reference" and res["target"] == "next-draw" and res["backend"] == "hip"
    assert (res["n_draws"], res["n_train"], res["n_val"]) == (20001, margin, n - margin)
    assert res["check_predicts"] is False and "false" in capsys.readouterr().out.split()  # unequal lengths
    assert res["workdir"] is None and res["checkpoint"] == path and res["world_size"] == 1
    d = generate_masks(20001, seed=4, planted=0.9)
    m = d.cpu().numpy()
    X, Y = unpack(m[:-1]).astype(np.float64), unpack(m[1:]).astype(np.float64)
    host = GBDT(eta=1.0, max_depth=3, gamma=1.0, nround=3, backend="hip")
    host.fit(X[:margin], Y[:margin], evals={"train": (X[:margin], Y[:margin]), "test": (X[margin:], Y[margin:])})
    assert res["train_logloss"] == host.history[-1]["train"] and res["val_logloss"] == host.history[-1]["test"]
    lg = torch.zeros(n - margin, 64, dtype=torch.float32, device="cuda")
    lg[:, :62] = torch.from_numpy(host.predict_margin(X[margin:]).astype(np.float32)).cuda()
    assert res["val"] == _finish(FM.draw_metrics(lg, d, n - margin, loss="bce", offset=margin))
    _aligned(res["val"], lg, Y[margin:])
    back = GBDT.load(path)
    assert back.n_tasks == 62 and back.num_feature == 62
    assert np.array_equal(back.predict(X[margin:margin + 300]), host.predict(X[margin:margin + 300], backend="numpy"))
    got = back.predict_margin_draw_masks(d, (margin, margin + 300)).cpu().numpy()  # (a loaded model: 0.5 splits)
    assert np.array_equal(got[:, :62], host.predict_margin(X[margin:margin + 300]).astype(np.float32))


@pytest.mark.parametrize("model", ["rf", "gbdt"])
def test_train_refuses_what_cannot_fit_before_allocating(model, tmp_path, monkeypatch):
    import torch

    from euromillioner_amd.data import device_gen
    from euromillioner_amd.train import train

    def no_masks(*a, **k):
        raise AssertionError("the masks were generated although the buffers cannot fit")

    free = 1 << 20
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (free, 288 << 30))
    monkeypatch.setattr(device_gen, "generate_masks", no_masks)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError) as e:
        train(_cfg(model, tmp_path, **{"rf.n_trees": 8, "gbdt.nround": 3}))
    assert torch.cuda.memory_allocated() == before
    text = str(e.value)
    need = [int(w) for w in text.replace(",", " ").split() if w.isdigit()]
    assert str(free) in text and any(v > free for v in need), text
