"""The count-table kernels (csrc/draw_counts.hip) and the model on the device.

Every comparison is exact equality: integer counts against ``pair_counts_np``, float32 logits bit for bit against
``logits_np`` (a fixed order of fp32 additions), metrics and back-test integers against the same kernels called by
hand.  The specification itself is tied to its definitions by tests/test_count_table_cpu.py."""
import json

import numpy as np
import pytest

from _count_table_cases import case_masks, random_table, valid_masks

from euromillioner_amd.models import count_table as CT

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025, 100003]  # one lane .. past a wave, a block's batch, several blocks


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _leave_the_device_as_found():
    """Hand the cached device memory back when this file is done, so that the timing guards that run later in the
    same process allocate from the state they would find without it."""
    yield
    import torch

    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big():
    """(host int64 [n], device copy) arbitrary masks, n past the largest window + the largest lag."""
    m = case_masks(100003 + 4 + 9, 21)
    return m, _dev(m)


# ----------------------------------------------------------------------------- pair counts
@pytest.mark.parametrize("lag", [0, 1, 2, 3, 4])
def test_pair_counts_equal_numpy(big, lag):
    import torch

    from euromillioner_amd.ops import draw_counts as DC

    m, d = big
    n = len(m)
    assert (m.view(np.uint64) >> np.uint64(62)).any() and (m == 0).any() and (m == -1).any()
    windows = [(d, m, 0, c) for c in COUNTS]
    windows += [(d, m, 9, None), (d, m, n - lag - 70, 70), (d[:lag + 1], m[:lag + 1], 0, None)]
    for dm, hm, first, count in windows:
        C = DC.pair_counts(dm, lag, first=first, count=count)
        c = len(hm) - lag - first if count is None else count
        assert C.dtype == torch.int64 and tuple(C.shape) == (64, 64) and C.is_cuda
        assert np.array_equal(C.cpu().numpy(), CT.pair_counts_np(hm, lag, first, c)), (lag, first, count)


def test_pair_counts_contention():
    """All masks identical: every lane of every wave hits the same cells."""
    from euromillioner_amd.ops import draw_counts as DC

    v = (1 << 0) | (1 << 17) | (1 << 49) | (1 << 50) | (1 << 61) | (3 << 62)
    hit = np.zeros(64, dtype=bool)
    hit[[0, 17, 49, 50, 61]] = True
    for count in (1, 64, 1000, 70001):
        d = _dev(np.full(count + 2, v, dtype=np.uint64).view(np.int64))
        for lag in (0, 2):
            C = DC.pair_counts(d, lag, 0, count).cpu().numpy()
            assert np.array_equal(C, np.where(hit[:, None] & hit[None, :], count, 0)), (count, lag)


def test_pair_counts_consistency(big):
    import torch

    from euromillioner_amd.ops import draw_counts as DC
    from euromillioner_amd.ops import tree_inputs as TI

    m, d = big
    C0 = DC.pair_counts(d, 0, 5, 50000).cpu().numpy()
    bc = TI.bit_counts(d, 5, 50005)
    assert np.array_equal(np.diag(C0)[:62], bc[:62]) and not np.diag(C0)[62:].any()
    a, b, whole = DC.pair_counts(d, 3, 0, 12345), DC.pair_counts(d, 3, 12345, 40000), DC.pair_counts(d, 3, 0, 52345)
    assert torch.equal(a + b, whole)
    assert torch.equal(DC.pair_counts(d, 3, 0, 52345), whole)
    v = _dev(valid_masks(3000, 4, planted=0.5))
    C = DC.pair_counts(v, 1, 0, 2999).cpu().numpy()
    assert np.array_equal(C.sum(1), 7 * TI.bit_counts(v, 0, 2999)) and np.array_equal(C.sum(0), 7 * TI.bit_counts(v, 1, 3000))


def test_pair_counts_refusals(big):
    import torch

    from euromillioner_amd.ops import draw_counts as DC

    m, d = big
    n = len(m)
    out = torch.full((64, 64), -7, dtype=torch.int64, device="cuda")
    for lag, first, count in ((1, 0, n), (1, n - 1, 1), (2, n - 3, 2), (5, 0, 1), (-1, 0, 1), (1, 0, 0), (1, -1, 3)):
        with pytest.raises(ValueError):
            DC.pair_counts(d, lag, first, count, out=out)
    for bad in (m, d.to(torch.int32), d.view(-1, 1)[:, 0][::2], torch.zeros(4, 4, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            DC.pair_counts(bad, 1, 0, 1, out=out)
    with pytest.raises(ValueError):
        DC.pair_counts(d, 1, 0, 10, out=out.to(torch.int32))
    with pytest.raises(ValueError):  # the C entry point refuses on its own as well
        from euromillioner_amd.ops import _native as N

        N.call("em_pair_counts", d.data_ptr(), n, n - 1, 1, 1, out.data_ptr(), N.stream_handle(d.device))
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    assert DC.pair_counts(d, 1, 0, 10, out=out) is out and int(out.sum()) > 0


# ----------------------------------------------------------------------------- logits
@pytest.fixture(scope="module")
def logit_masks():
    m = case_masks(1400, 33)
    return m, _dev(m)


@pytest.mark.parametrize("lags", [1, 2, 3, 4])
def test_count_logits_equal_numpy_bit_for_bit(logit_masks, lags):
    import torch

    from euromillioner_amd.ops import draw_counts as DC

    m, d = logit_masks
    n = len(m)
    table, prior = random_table(lags, 40 + lags)
    dt, dp = _dev(table), _dev(prior)
    g = np.random.default_rng(lags)
    for B in (1, 63, 64, 65, 257, 1025):
        for offset in (0, 7):
            got = DC.count_logits(d, B, dt, dp, offset=offset)
            assert got.dtype == torch.float32 and tuple(got.shape) == (B, 64)
            want = CT.logits_np(m, offset + np.arange(B), table, prior)
            assert np.array_equal(got.cpu().numpy(), want), (lags, B, offset)
            assert not got[:, 62:].any()
        idx = g.integers(0, n - lags, size=B).astype(np.int32)
        idx[-1] = idx[0]  # a repeat
        idx[B // 2] = n - lags - 1  # the last valid sample
        got = DC.count_logits(d, B, dt, dp, sidx=_dev(idx))
        assert np.array_equal(got.cpu().numpy(), CT.logits_np(m, idx, table, prior)), (lags, B, "sidx")
    # a strided out: 68 floats between rows, the 4 columns past 64 untouched
    B = 257
    buf = torch.full((B, 68), -3.0, dtype=torch.float32, device="cuda")
    ret = DC.count_logits(d, B, dt, dp, offset=3, out=buf)
    assert ret is buf
    assert np.array_equal(buf[:, :64].cpu().numpy(), CT.logits_np(m, 3 + np.arange(B), table, prior))
    assert bool((buf[:, 64:] == -3.0).all())
    # the last valid sample is accepted, one past it is refused
    last = n - lags - 1
    assert np.array_equal(DC.count_logits(d, 1, dt, dp, offset=last).cpu().numpy(), CT.logits_np(m, [last], table, prior))
    assert np.array_equal(DC.count_logits(d, 5, dt, dp, offset=last - 4).cpu().numpy(),
                          CT.logits_np(m, last - 4 + np.arange(5), table, prior))
    with pytest.raises(ValueError):
        DC.count_logits(d, 1, dt, dp, offset=last + 1)
    with pytest.raises(ValueError):
        DC.count_logits(d, 6, dt, dp, offset=last - 4)
    with pytest.raises(ValueError):
        DC.count_logits(d, 2, dt, dp, sidx=_dev(np.array([0, last + 1], dtype=np.int32)))


@pytest.mark.parametrize("lags", [1, 2, 3, 4])
def test_count_logits_sparse_chunks_bit_for_bit(lags):
    """Chunks whose masks all have at most 8 set bits take the packed-index path (unused slots add -0.0f): 0 to
    8 bits per mask, stray bits 62-63, and signed zeros in the table and the prior, compared as bit patterns."""
    from euromillioner_amd.ops import draw_counts as DC

    g = np.random.default_rng(70 + lags)
    n = 700
    m = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        bits = g.choice(62, size=int(g.integers(0, 9)), replace=False)
        m[i] = np.bitwise_or.reduce(np.uint64(1) << bits.astype(np.uint64), initial=np.uint64(0))
        m[i] |= np.uint64(int(g.integers(0, 4)) << 62)
    m[5:9] = np.uint64(3 << 62)  # no draw bits at all
    m[9] = np.uint64(0xFF | (3 << 62))  # exactly 8
    m[200:264] = np.uint64((1 << 61) | 1)
    m = m.view(np.int64)
    table, prior = random_table(lags, 90 + lags)
    table[:, ::3, ::5] = -0.0
    table[:, 1, :62] = 0.0
    prior[::4] = -0.0
    prior[62:] = 0.0
    d, dt, dp = _dev(m), _dev(table), _dev(prior)
    for B, offset in ((n - lags, 0), (129, 64), (1, 5)):
        got = DC.count_logits(d, B, dt, dp, offset=offset).cpu().numpy()
        want = CT.logits_np(m, offset + np.arange(B), table, prior)
        assert np.array_equal(got[:, :62].view(np.uint32), want[:, :62].view(np.uint32)), (lags, B, offset)
        assert not got[:, 62:].any()
    # one dense mask sends its chunk down the scalar walk: the same rows, the same bits
    m2 = m.copy()
    m2[70] = -1
    got = DC.count_logits(_dev(m2), 300, dt, dp).cpu().numpy()
    want = CT.logits_np(m2, np.arange(300), table, prior)
    assert np.array_equal(got[:, :62].view(np.uint32), want[:, :62].view(np.uint32))


def test_count_logits_on_fitted_weights_and_refusals(logit_masks):
    import torch

    from euromillioner_amd.ops import draw_counts as DC

    m, d = logit_masks
    model = CT.CountTable(2, 1.0, "cpu").fit_masks_np(m)
    dt, dp = _dev(model.table), _dev(model.prior)
    got = DC.count_logits(d, 1398, dt, dp)
    assert np.array_equal(got.cpu().numpy(), model.logits_np(m, np.arange(1398)))
    out = torch.full((8, 64), 5.0, dtype=torch.float32, device="cuda")
    bad = [dict(table=dt[:, :32]), dict(table=dt.double()), dict(prior=dp[:62]), dict(table=dt.cpu()),
           dict(B=0), dict(offset=-1), dict(out=out[:, :32]), dict(out=torch.zeros(8, 67, device="cuda")),
           dict(out=out.double()), dict(sidx=_dev(np.zeros(3, dtype=np.int32))), dict(sidx=_dev(np.zeros(8, dtype=np.int64))),
           dict(sidx=_dev(np.array([0, 1, 2, 3, 4, 5, 6, -1], dtype=np.int32)))]
    for kw in bad:
        args = dict(B=8, table=dt, prior=dp, offset=0, sidx=None, out=out)
        args.update(kw)
        with pytest.raises(ValueError):
            DC.count_logits(d, args["B"], args["table"], args["prior"], offset=args["offset"], sidx=args["sidx"],
                            out=args["out"])
    with pytest.raises(ValueError):
        DC.count_logits(d[:2], 1, dt, dp)  # two draws cannot hold two lags and a target
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


# ----------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def planted():
    m = valid_masks(6000, 5, planted=0.9)
    return m, _dev(m)


@pytest.mark.parametrize("lags", [1, 3])
def test_model_fit_on_the_device_equals_the_numpy_fit(planted, lags, tmp_path):
    import torch

    from euromillioner_amd.ops import fused_mlp as FM

    m, d = planted
    first, count = 2, 4000
    dev = CT.CountTable(lags, 0.5, "cuda").fit_draw_masks(d, first, count)
    ref = CT.CountTable(lags, 0.5, "cpu").fit_masks_np(d.cpu().numpy(), first, count)
    assert dev.backend_used == "hip" and ref.backend_used == "numpy" and dev.N == ref.N == count
    for k in ("counts", "S", "T", "table", "prior"):
        assert np.array_equal(getattr(dev, k), getattr(ref, k)), k
    # evaluate == draw_metrics summed by hand on count_logits' output
    a, B = first + count, len(m) - lags - (first + count)
    lg = dev.logits(d, B, offset=a)
    assert np.array_equal(lg.cpu().numpy(), ref.logits_np(m, a + np.arange(B)))
    tot = FM.draw_metrics(lg, d[lags - 1:], B, loss="softmax", offset=a).double().sum(0).cpu().numpy()
    ev = dev.evaluate(d, B, offset=a)
    ev3 = dev.evaluate(d, B, offset=a, chunk=512)  # whole metric blocks: the same fp32 partials, regrouped in fp64
    assert ev["count"] == B == int(tot[7]) == ev3["count"]
    for i, k in enumerate(FM.METRIC_NAMES[:-1]):
        assert ev[k] == float(tot[i] / tot[7]), k
        assert abs(ev3[k] - ev[k]) <= 1e-12 * max(1.0, abs(ev[k])), k
    if lags == 1:
        assert ev["hits_main"] > 4.0 and ev["hits_star"] > 1.5
    # a saved and re-loaded model gives identical logits
    path = str(tmp_path / "m.cnt")
    dev.save(path)
    again = CT.CountTable.load(path, "cuda")
    assert torch.equal(again.logits(d, B, offset=a), lg)
    sidx = _dev(np.array([a + 5, a, a + 5, len(m) - lags - 1], dtype=np.int32))
    assert torch.equal(again.logits(d, 4, sidx=sidx), lg[[5, 0, 5, B - 1]])


def test_model_fit_from_rows_uses_the_gpu():
    from euromillioner_amd.data.draws import mask_bits
    from euromillioner_amd.data.synthetic import generate_draws

    nums = generate_draws(700, seed=8, planted=0.5)[0]
    dev = CT.CountTable(2).fit(nums)
    ref = CT.CountTable(2, device="cpu").fit(nums)
    assert dev.backend_used == "hip" and ref.backend_used == "numpy"
    assert np.array_equal(dev.counts, ref.counts) and np.array_equal(dev.table, ref.table)
    assert np.array_equal(dev.prior, ref.prior) and dev.N == ref.N == 698
    assert np.array_equal(ref.counts[0], CT.pair_counts_np(mask_bits(nums), 1, 1, 698))


def test_model_backtest_and_tickets(planted):
    import torch

    from euromillioner_amd.ops import tickets as OT

    m, d = planted
    lags = 2
    model = CT.CountTable(lags, 1.0, "cuda").fit_draw_masks(d, 0, 4000)
    a, B, nt = 4000, 1500, 4
    lg = model.logits(d, B, offset=a)
    r = OT.draw_tickets(lg, B, nt, 0.7, 9, masks=d[lags - 1:], offset=a, want_tickets=False)
    hist, best = OT.sum_partials(r["partials"])
    for chunk in (1 << 20, 512, 333):
        bt = model.backtest(d, B, nt, 0.7, 9, offset=a, chunk=chunk)
        assert np.array_equal(bt["hist"], hist) and np.array_equal(bt["best"], best), chunk
        assert bt["rows"] == B and bt["tickets"] == B * nt and int(bt["hist"].sum()) == B * nt
    tk = model.tickets(d, B, nt, 0.7, 9, offset=a)
    assert torch.equal(tk, OT.draw_tickets(lg, B, nt, 0.7, 9, offset=a)["tickets"])
    assert model.group is None


# ----------------------------------------------------------------------------- end to end
def test_cli_train_on_device_draws(capsys, tmp_path):
    from euromillioner_amd.cli import main

    path = str(tmp_path / "dev.cnt")
    capsys.readouterr()
    rc = main(["train", "--model", "counts", "--data-source", "device", "--n-draws", "20000", "--planted", "0.9",
               "--ckpt", path, "--log-level", "ERROR"])
    res = json.loads(capsys.readouterr().out.splitlines()[-1])
    assert rc == 0 and res["backend"] == "hip" and res["model"] == "counts"
    assert list(res) == ["model", "backend", "lags", "alpha", "train_samples", "val_samples", "seconds", "val",
                         "checkpoint"]
    assert res["train_samples"] == int(0.7 * 19999) and res["val_samples"] == 19999 - res["train_samples"]
    assert res["val"]["hits_main"] > 4.0 and res["val"]["count"] == res["val_samples"]
    assert CT.CountTable.load(path).N == res["train_samples"]
    capsys.readouterr()
    rc = main(["backtest", "--ckpt", path, "--tickets", "2", "--n-draws", "3000", "--planted", "0.9", "--log-level",
               "ERROR"])
    bt = json.loads(capsys.readouterr().out.splitlines()[-1])
    assert rc == 0 and bt["engine"] == "hip" and bt["model"] == "counts" and bt["rows"] == 2999 - int(0.7 * 2999)
