"""Random forest out-of-bag evaluation on the device (csrc/forest.hip K11-OOB: rf_predict<true>,
rf_predict_lds<G, true>, rf_oob_metrics) against the fp64 reference written from the definition
(tests/_rf_oob_ref.py).  The forests are the numpy engine's (shared with tests/test_rf_oob_cpu.py), so
every difference is the OOB kernels'."""
import numpy as np
import pytest

import _rf_oob_ref as R

pytestmark = pytest.mark.gpu


def _device_oob(name, stream_trees):
    from euromillioner_amd.ops import forest as K

    rf, X, Y, rp, rc = R.build_case(name)
    start = R.CASES[name][5] or 0
    return K.oob_predict(X, rf.feat, rf.value, rf.max_depth, rf.seed, start, stream_trees=stream_trees)


@pytest.mark.parametrize("name", list(R.CASES))
def test_device_oob_matches_reference(name):
    """Both forms (the streamed one applies to one-word rows at depth <= 8, otherwise both calls take the
    general kernel): counts exact, probabilities within (count + 2) * 2^-24, zero-count rows and outputs
    62 / 63 all zero, and the two forms bit-identical."""
    import torch

    from euromillioner_amd.ops import _native as N

    rf, X, Y, rp, rc = R.build_case(name)
    streamed_applies = N.lib().em_rf_predict_scratch(X.shape[1], len(rf.feat), rf.max_depth) > 0
    assert streamed_applies == (name not in ("d6_lags2", "d9"))
    out_s, cnt_s = _device_oob(name, True)
    out_g, cnt_g = _device_oob(name, False)
    assert out_s.shape == (len(X), 64) and out_s.dtype == torch.float32 and cnt_s.dtype == torch.int32
    for out, cnt in ((out_s, cnt_s), (out_g, cnt_g)):
        worst = R.check_oob(out.cpu().numpy(), cnt.cpu().numpy(), rp, rc)
        print(f"{name}: worst error / budget {worst:.3f}, zero-count rows {int((rc == 0).sum())}")
    assert torch.equal(out_s, out_g) and torch.equal(cnt_s, cnt_g)


@pytest.mark.parametrize("depth,trees,n,t_off", [(8, 100, 200001, 0), (3, 37, 600000, 5)])
def test_device_oob_streamed_two_row_groups(depth, trees, n, t_off):
    """The streamed kernel with two row groups per wave (every case above has at most 3000 rows: one group)
    equals the one-wave-per-row kernel bit for bit, `out` and `count`; `count` equals the specification's
    (models/forest.py poisson_weights == 0, summed over the trees); outputs 62 / 63 and zero-count rows are
    zero.  On 256 CUs: 66 rows per wave (the second group holds 2 live lanes in most waves and none in the
    last), and 128 rows per wave on a grid past one workgroup per CU with a tree offset.  The out-of-bag sets
    depend on (seed, tree id, row) only, so the trees need not have been fitted on these rows."""
    import torch

    from euromillioner_amd.data.draws import mask_bits
    from euromillioner_amd.data.synthetic import generate_draws
    from euromillioner_amd.models.forest import poisson_weights
    from euromillioner_amd.ops import forest as K

    # the launcher's shape (csrc/forest.hip rf_predict_streamed): 12 waves, one workgroup per CU, <= 128 rows per wave
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = min(-(-n // (64 * 12)), cus)
    rows_per_wave = min(-(-(-(-n // grid)) // 12), 128)
    if rows_per_wave <= 64:
        pytest.skip(f"{cus} CUs give {rows_per_wave} rows per wave at {n} rows: one row group")
    seed = 3
    nums, _ = generate_draws(20001, seed=1, planted=0.9, native=False)
    md = torch.from_numpy(mask_bits(nums).view(np.int64)).cuda()
    n_tr = 14000
    feat, value, _, _ = K.fit(md[:n_tr].reshape(-1, 1).contiguous(), md[1:n_tr + 1].contiguous(), 62, t_off, trees,
                              depth, 8, 1, True, seed, return_device=True)
    g = torch.Generator(device="cuda").manual_seed(n)
    Xv = md[torch.randint(0, 20000, (n,), device="cuda", generator=g)].reshape(-1, 1).contiguous()
    out_s, cnt_s = K.oob_predict(Xv, feat, value, depth, seed, t_off, stream_trees=True)
    out_g, cnt_g = K.oob_predict(Xv, feat, value, depth, seed, t_off, stream_trees=False)
    assert torch.equal(out_s, out_g) and torch.equal(cnt_s, cnt_g)
    spec = np.zeros(n, dtype=np.int32)
    for t in range(trees):
        spec += poisson_weights(seed, t_off + t, n) == 0
    cnt = cnt_s.cpu().numpy()
    print(f"rows per wave {rows_per_wave}, count {cnt.min()}..{cnt.max()}, zero-count rows {int((cnt == 0).sum())}")
    assert np.array_equal(cnt, spec)
    assert bool((out_s[:, 62:] == 0).all()) and bool((out_s[cnt_s == 0] == 0).all())


@pytest.mark.parametrize("name", ["d5", "t3_d8", "n1537"])
def test_device_metrics_match_reference(name):
    """em_rf_oob_metrics against the definition applied to the device's own fp32 probabilities: every integer
    equal, the Brier and log-loss sums within k * 2^-24 * sum |term|."""
    from euromillioner_amd.ops import forest as K

    rf, X, Y, rp, rc = R.build_case(name)
    out, cnt = _device_oob(name, True)
    got = K.oob_totals(out, cnt, Y)
    ref = R.metrics_reference(out.cpu().numpy(), cnt.cpu().numpy(), Y)
    assert ref["rows"] == int((rc > 0).sum()) and ref["rows"] < len(X)
    R.check_totals(got, ref)
    R.check_score(K.oob_metrics(out, cnt, Y), R.finish_reference(ref))


def test_device_metrics_ties_pick_the_earlier_index():
    """All outputs equal: the pick must be outputs 0..4 and 50, 51 (csrc/draw_topk.h's stable order)."""
    import torch

    from euromillioner_amd.ops import forest as K

    n = 300  # two blocks, the second partial
    out = torch.full((n, 64), 0.25, device="cuda")
    out[:, 62:] = 0
    cnt = torch.ones(n, dtype=torch.int32, device="cuda")
    cnt[7] = 0
    first = np.uint64(sum(1 << j for j in (0, 1, 2, 3, 4, 50, 51)))
    later = np.uint64(sum(1 << j for j in (5, 6, 7, 8, 9, 52, 53)))
    tot = K.oob_totals(out, cnt, np.full(n, first, dtype=np.uint64))
    assert tot["rows"] == n - 1 and tot["exact"] == n - 1 and tot["mismatch_bits"] == 0
    assert tot["hits_main"] == 5 * (n - 1) and tot["hits_star"] == 2 * (n - 1) and tot["min_trees"] == 1
    tot = K.oob_totals(out, cnt, np.full(n, later, dtype=np.uint64))
    assert tot["hits_main"] == 0 and tot["hits_star"] == 0 and tot["mismatch_bits"] == 14 * (n - 1)


def test_forest_oob_score_device_vs_cpu():
    """RandomForest(device="cuda"): fit, OOB prediction and metrics on the device, against the numpy forest's."""
    from euromillioner_amd.models.forest import RandomForest

    rf, X, Y, rp, rc = R.build_case("d5")
    _, _, F = R._cache["data", 1]
    gpu = RandomForest(n_trees=10, max_depth=5, seed=11, device="cuda").fit(X, Y, F)
    assert gpu.backend_used == "hip" and np.array_equal(gpu.feat, rf.feat)
    proba, count = gpu.oob_predict_proba(X)
    assert proba.shape == (len(X), 62) and proba.dtype == np.float32 and count.dtype == np.int32
    R.check_oob(proba, count, rp, rc)
    cp, cc = rf.oob_predict_proba(X)
    ref = R.finish_reference(R.metrics_reference(cp, cc, Y))
    R.check_score(rf.oob_score(X, Y), ref)
    R.check_score(gpu.oob_score(X, Y), ref)
    with pytest.raises(ValueError):
        gpu.oob_predict_proba(X[:-1])


def test_bad_arguments_return_the_error_code():
    """EM_ERR_ARG (-1) before any launch: the output buffers keep their fill."""
    import torch

    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.ops import forest as K  # noqa: F401  (registers the signatures)

    lib = N.lib()
    n, T, depth = 64, 4, 2
    nodes = (1 << (depth + 1)) - 1
    X = torch.zeros(n, dtype=torch.int64, device="cuda")
    feat = torch.full((T, nodes), -1, dtype=torch.int16, device="cuda")
    value = torch.zeros(T, nodes, 64, device="cuda")
    out = torch.full((n, 64), 7.0, device="cuda")
    cnt = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = N.stream_handle(torch.device("cuda"))

    def call(**kw):
        a = dict(X=X.data_ptr(), W=1, N=n, feat=feat.data_ptr(), value=value.data_ptr(), T=T, depth=depth, seed=1,
                 t_off=0, out=out.data_ptr(), ldo=64, count=cnt.data_ptr(), prep=None)
        a.update(kw)
        return lib.em_rf_oob_predict(a["X"], a["W"], a["N"], a["feat"], a["value"], a["T"], a["depth"], a["seed"],
                                     a["t_off"], a["out"], a["ldo"], a["count"], a["prep"], st)

    for bad in (dict(X=None), dict(feat=None), dict(value=None), dict(out=None), dict(count=None), dict(W=0),
                dict(N=-1), dict(T=-1), dict(ldo=63), dict(depth=-1), dict(depth=15), dict(t_off=-1),
                dict(t_off=2**31 - 2)):
        assert call(**bad) == -1, bad
    Y = torch.zeros(n, dtype=torch.int64, device="cuda")
    part = torch.full((N.query("em_rf_oob_metrics_words", n),), 7, dtype=torch.int64, device="cuda")
    assert part.numel() == 10 and N.query("em_rf_oob_metrics_words", -1) == -1

    def mcall(**kw):
        a = dict(p=out.data_ptr(), ldo=64, c=cnt.data_ptr(), Y=Y.data_ptr(), N=n, part=part.data_ptr())
        a.update(kw)
        return lib.em_rf_oob_metrics(a["p"], a["ldo"], a["c"], a["Y"], a["N"], a["part"], st)

    for bad in (dict(p=None), dict(c=None), dict(Y=None), dict(part=None), dict(ldo=61), dict(N=-1)):
        assert mcall(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((cnt == 7).all()) and bool((part == 7).all())
    assert call() == 0 and call(N=0) == 0 and mcall(N=0) == 0  # the same buffers with good arguments
    torch.cuda.synchronize()
    assert bool((cnt <= T).all()) and bool((out[:, 62:] == 0).all())
