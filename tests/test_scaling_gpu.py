"""em_scaling_stats / em_scaling_apply (csrc/calibration_fit.hip) and what is built on them, against the fp64
reference tests/_scaling_ref.py fed the SAME fp32 logits.

Cases: B in (1, 63, 64, 65, 255, 256, 257, 513), both heads, the three parameter points of ``_scaling_ref.POINTS``;
each once with offset 17 and a row stride of 64, once through a sample index with repeats and a stride of 68, once
with offset 0 and a stride of 72.  The logits hold rows at +-120, the masks draws without a main or a star; columns
62 and up, and every row at or past B, hold NaN; every output sits between poisoned guard rows.  Rules:

* the fp64 sum of the partials, and every block's partials, are within ``2 K u A`` of the reference
  (``_scaling_ref``: K = 72 derived there, doubled as in tests/_adam_ref.py);
* the partials of B = 513 are bit-equal to those of its three blocks run alone, and bit-equal run to run;
* ``apply_scaling`` is bit-equal to ``scaling.apply_np``, in place and out of place, pads 0, nothing else written;
* a refused call raises and leaves the poisoned outputs bit-unchanged;
* ``fit_device`` stops where the reference gradient vanishes as far as fp32 partials can tell: every component is
  within ``2 K u A`` of that component plus ``|H| ulp`` (the change one float32 ulp of a parameter makes), and within
  standardised distance 5 of the planted parameters.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import _scaling_ref as SR

pytestmark = pytest.mark.gpu

HEADS = ("softmax", "bce")
POISON = -7.5
# (offset, sidx seed, row stride)
FORMS = ((17, None, 64), (0, 2, 68), (0, None, 72))


@pytest.fixture(scope="module")
def dev_masks():
    return torch.from_numpy(SR.inputs()[1].copy()).cuda()


def _device_logits(z: np.ndarray, B: int, ld: int) -> torch.Tensor:
    """Rows [0, B) of z in a NaN-filled [B + 3, ld] buffer: NaN in columns 62.. and in the rows at and past B."""
    buf = torch.full((B + 3, ld), float("nan"), dtype=torch.float32)
    buf[:B, :62] = torch.from_numpy(z[:B, :62].copy())
    return buf.cuda()[:, :64]


def _guarded(nb: int):
    big = torch.full((nb + 2, 2, 6), POISON, dtype=torch.float32, device="cuda")
    return big, big[1:-1]


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("loss", HEADS)
def test_stats_match_reference(dev_masks, loss):
    from euromillioner_amd.ops import calibration_fit as CF

    z, _ = SR.inputs()
    worst = 0.0
    for B in SR.BS:
        for off, seed, ld in FORMS:
            lg = _device_logits(z, B, ld)
            assert lg.stride(0) == ld
            sidx = torch.from_numpy(SR.sample_index(B, seed)).cuda() if seed is not None else None
            for p, (a, b) in enumerate(SR.POINTS[loss]):
                what = f"{loss} B={B} offset={off} sidx={seed} ld={ld} a={a} b={b}"
                S, A = SR.case_reference(loss, p, B, off, seed)
                big, out = _guarded(CF.scaling_blocks(B))
                parts = CF.scaling_stats(lg, dev_masks, B, loss, a, b, offset=off, sidx=sidx, out=out)
                again = CF.scaling_stats(lg, dev_masks, B, loss, a, b, offset=off, sidx=sidx)
                torch.cuda.synchronize()
                assert parts.shape == ((B + 255) // 256, 2, 6) and parts.data_ptr() == out.data_ptr()
                assert bool((big[0] == POISON).all()) and bool((big[-1] == POISON).all()), what + ": guard written"
                assert _bits_equal(parts, again), what
                got = parts.double().cpu().numpy()
                assert np.isfinite(got).all(), what
                Sb, Ab = SR.block_sums(S), SR.block_sums(A)
                ok = SR.within(got, Sb, Ab)
                assert ok.all(), (what, "per block", got[~ok], Sb[~ok], SR.budget(Ab)[~ok])
                tot = CF.sum_scaling(parts)
                assert tot.dtype == np.float64 and tot.shape == (2, 6)
                ok = SR.within(tot, S.sum(0), A.sum(0))
                assert ok.all(), (what, "total", tot[~ok], S.sum(0)[~ok])
                if loss == "softmax":
                    assert not got[:, :, [2, 4, 5]].any(), what
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst = max(worst, float(np.nanmax(np.abs(got - Sb) / SR.budget(Ab))))
    print(f"{loss}: the kernel uses at most {worst:.4f} of the budget K u A (2 allowed)")


@pytest.mark.parametrize("loss", HEADS)
def test_blocks_alone_give_the_same_bits(dev_masks, loss):
    from euromillioner_amd.ops import calibration_fit as CF

    z, _ = SR.inputs()
    lg = _device_logits(z, 513, 64)
    a, b = SR.POINTS[loss][1]
    whole = CF.scaling_stats(lg, dev_masks, 513, loss, a, b, offset=17)
    assert _bits_equal(whole, CF.scaling_stats(lg, dev_masks, 513, loss, a, b, offset=17))
    for k, rows in enumerate((256, 256, 1)):
        alone = CF.scaling_stats(lg[256 * k:], dev_masks, rows, loss, a, b, offset=17 + 256 * k)
        assert _bits_equal(alone[0], whole[k]), (loss, k)


def test_draw_metrics_identities(dev_masks):
    """At a = 1, b = 0 the L sums are the ``loss`` column of em_draw_metrics: over rows under softmax, over 62 x rows
    under bce (rows whose groups all hold a target bit; both sides are fp32 partials, each within its budget)."""
    from euromillioner_amd.ops import calibration_fit as CF
    from euromillioner_amd.ops.fused_mlp import draw_metrics

    z, m = SR.inputs()
    Y = SR.bits(m[1:514])
    keep = np.flatnonzero((Y[:, :50].sum(1) > 0) & (Y[:, 50:].sum(1) > 0)).astype(np.int32)
    B = len(keep)
    lg = torch.from_numpy(np.nan_to_num(z[keep], nan=0.0)).cuda()
    sidx = torch.from_numpy(keep).cuda()
    for loss in HEADS:
        S, A = SR.reference(z[keep], Y[keep], loss)
        tot = CF.sum_scaling(CF.scaling_stats(lg, dev_masks, B, loss, sidx=sidx))
        dm = draw_metrics(lg, dev_masks, B, loss=loss, sidx=sidx).double().sum(0).cpu().numpy()
        assert int(dm[7]) == B
        scale = 1.0 if loss == "softmax" else 62.0
        allow = SR.FACTOR * SR.budget(A[:, 0].sum())
        assert abs(tot[:, 0].sum() - S[:, 0].sum()) <= allow
        assert abs(dm[0] * scale - S[:, 0].sum()) <= allow, (loss, dm[0] * scale, S[:, 0].sum())
        assert abs(dm[0] * scale - tot[:, 0].sum()) <= 2 * allow


def test_apply_is_bit_equal_to_the_specification():
    from euromillioner_amd import scaling as SC
    from euromillioner_amd.ops import calibration_fit as CF

    z, _ = SR.inputs()
    for B in SR.BS:
        for ld, ldo in ((64, 64), (68, 72), (72, 64)):
            for a, b in (((1.0, 1.0), (0.0, 0.0)), ((0.3, 1.7), (0.7, -0.1)), ((4.0, 0.25), (-3.0, 3.0))):
                what = f"B={B} ld={ld} ldo={ldo} a={a} b={b}"
                lg = _device_logits(z, B, ld)
                want = SC.apply_np(z[:B], a, b)
                big = torch.full((B + 2, ldo), POISON, dtype=torch.float32, device="cuda")
                out = CF.apply_scaling(lg, B, a, b, out=big[1:-1, :64])
                torch.cuda.synchronize()
                assert out.data_ptr() == big[1].data_ptr()
                got = big.cpu().numpy()
                assert np.array_equal(got[1:-1, :64].view(np.int32), want.view(np.int32)), what
                assert (got[0] == POISON).all() and (got[-1] == POISON).all() and (got[:, 64:] == POISON).all(), what
                fresh = CF.apply_scaling(lg, B, a, b)
                assert fresh.shape == (B, 64) and np.array_equal(fresh.cpu().numpy().view(np.int32), want.view(np.int32))
                # in place: the rows at and past B keep their NaN, the columns past 64 too
                before = lg.clone()
                same = CF.apply_scaling(lg, B, a, b, out=lg)
                torch.cuda.synchronize()
                assert same.data_ptr() == lg.data_ptr()
                assert np.array_equal(lg[:B].cpu().numpy().view(np.int32), want.view(np.int32)), what + " in place"
                assert _bits_equal(lg[B:], before[B:]), what


def test_refusals_leave_outputs_untouched(dev_masks):
    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.ops import calibration_fit as CF

    B = 300
    z, _ = SR.inputs()
    lg = torch.from_numpy(np.nan_to_num(z[:B], nan=0.0)).cuda()
    big, out = _guarded(CF.scaling_blocks(B))
    obig = torch.full((B + 2, 64), POISON, dtype=torch.float32, device="cuda")
    n = dev_masks.shape[0]
    sidx = torch.arange(B, dtype=torch.int32, device="cuda")
    nan, inf = float("nan"), float("inf")
    bad_calls = [
        dict(loss="hinge"), dict(a=(0.0, 1.0)), dict(a=(1.0, -2.0)), dict(a=(nan, 1.0)), dict(a=(1.0, inf)), dict(a=(1.0,)),
        dict(b=(nan, 0.0)), dict(b=(0.0, -inf)), dict(loss="softmax", b=(0.0, 0.5)), dict(B=0), dict(B=-1), dict(B=B + 1),
        dict(offset=-1), dict(offset=n - B), dict(logits=lg.cpu()), dict(logits=lg.double()), dict(logits=lg[:, :62]),
        dict(logits=torch.zeros(B, 66, device="cuda")[:, :64]),
        dict(logits=torch.zeros(B * 64 + 4, device="cuda")[1:B * 64 + 1].view(B, 64)),
        dict(masks=dev_masks.cpu()), dict(masks=dev_masks.int()), dict(sidx=sidx.long()), dict(sidx=sidx[:B - 1]),
        dict(sidx=sidx + (n - B)), dict(sidx=sidx - 1), dict(sidx=sidx.cpu()), dict(out=out[:1]), dict(out=out.double()),
    ]
    for kw in bad_calls:
        args = dict(logits=lg, masks=dev_masks, B=B, loss="bce", a=(1.0, 1.0), b=(0.0, 0.0), offset=0, sidx=None, out=out)
        args.update(kw)
        with pytest.raises(ValueError):
            CF.scaling_stats(args["logits"], args["masks"], args["B"], args["loss"], args["a"], args["b"],
                             offset=args["offset"], sidx=args["sidx"], out=args["out"])
        if set(kw) & {"loss", "B", "offset", "logits", "masks", "sidx"} and "b" not in kw:
            with pytest.raises(ValueError):
                CF.fit_device(args["logits"], args["masks"], args["B"], args["loss"], offset=args["offset"],
                              sidx=args["sidx"])
    for kw in (dict(a=(0.0, 1.0)), dict(a=(1.0, nan)), dict(b=(inf, 0.0)), dict(B=0), dict(B=B + 1),
               dict(logits=lg.cpu()), dict(logits=lg[:, :62]), dict(out=obig[1:-1].double()), dict(out=obig[1:-1, :60]),
               dict(out=obig[1:3]), dict(out=torch.zeros(B, 66, device="cuda")[:, :64]), dict(out=obig[1:-1].cpu())):
        args = dict(logits=lg, B=B, a=(1.0, 1.0), b=(0.0, 0.0), out=obig[1:-1])
        args.update(kw)
        with pytest.raises(ValueError):
            CF.apply_scaling(args["logits"], args["B"], args["a"], args["b"], out=args["out"])
    torch.cuda.synchronize()
    assert bool((big == POISON).all()) and bool((obig == POISON).all()), "written by a refused call"

    # raw calls: EM_ERR_ARG before any launch
    def pair(x, y):
        buf = (ctypes.c_float * 2)(x, y)
        return buf, ctypes.cast(buf, ctypes.c_void_p)

    keep = [pair(1.0, 1.0), pair(0.0, 0.0), pair(0.0, 1.0), pair(-1.0, 1.0), pair(nan, 1.0), pair(1.0, inf), pair(0.5, 0.0),
            pair(nan, 0.0), pair(0.0, -inf)]
    one, zero, a_zero, a_neg, a_nan, a_inf, b_half, b_nan, b_inf = (k[1] for k in keep)
    st = N.stream_handle(lg.device)
    good = [lg.data_ptr(), 64, dev_masks.data_ptr(), None, B, 0, 1, one, zero, out.data_ptr(), st]
    raw_bad = [(0, None), (2, None), (7, None), (8, None), (9, None), (1, 60), (1, 66), (1, 63), (4, 0), (4, -5),
               (4, 2 ** 31 - 1), (4, 2 ** 40), (5, -1), (0, lg.data_ptr() + 4), (6, 2), (6, -1), (7, a_zero), (7, a_neg),
               (7, a_nan), (7, a_inf), (8, b_nan), (8, b_inf)]
    for pos, val in raw_bad:
        args = list(good)
        args[pos] = val
        with pytest.raises(ValueError):
            N.call("em_scaling_stats", *args)
    soft = list(good)
    soft[6], soft[8] = 0, b_half  # a shift under the softmax head
    with pytest.raises(ValueError):
        N.call("em_scaling_stats", *soft)
    o = obig[1:-1]
    good_apply = [lg.data_ptr(), 64, B, one, zero, o.data_ptr(), 64, st]
    for pos, val in [(0, None), (5, None), (3, None), (4, None), (1, 60), (1, 66), (6, 62), (6, 65), (2, 0), (2, -1),
                     (2, 2 ** 31 - 1), (0, lg.data_ptr() + 4), (5, o.data_ptr() + 8), (3, a_zero), (3, a_nan),
                     (3, a_inf), (4, b_nan), (4, b_inf)]:
        args = list(good_apply)
        args[pos] = val
        with pytest.raises(ValueError):
            N.call("em_scaling_apply", *args)
    in_place = [lg.data_ptr(), 64, B, one, zero, lg.data_ptr(), 68, st]  # in place with another stride
    with pytest.raises(ValueError):
        N.call("em_scaling_apply", *in_place)
    torch.cuda.synchronize()
    assert bool((big == POISON).all()) and bool((obig == POISON).all()), "written by a refused raw call"
    assert CF.scaling_blocks(0) == 0 and CF.scaling_blocks(256) == 1 and CF.scaling_blocks(257) == 2
    assert CF.scaling_blocks(2 ** 31 - 1) == 0 and CF.scaling_blocks(-3) == 0
    # and the good calls do write
    N.call("em_scaling_stats", *good)
    N.call("em_scaling_apply", *good_apply)
    torch.cuda.synchronize()
    assert bool((big[0] == POISON).all()) and bool((big[-1] == POISON).all()) and bool((out != POISON).all())
    assert bool((obig[0] == POISON).all()) and bool((obig[-1] == POISON).all()) and bool((o != POISON).all())


def _gradient_vanishes(S, A, a, b, what):
    """Every component of the reference gradient is within 2 K u A of that component plus |H| ulp."""
    ulp_a, ulp_b = float(np.spacing(np.float32(abs(a)))), float(np.spacing(np.float32(abs(b))))
    allow_a = SR.FACTOR * SR.budget(A[1]) + S[3] * ulp_a + abs(S[4]) * ulp_b
    allow_b = SR.FACTOR * SR.budget(A[2]) + abs(S[4]) * ulp_a + S[5] * ulp_b
    print(f"{what}: g_a {S[1]:.3e} (allowed {allow_a:.3e})  g_b {S[2]:.3e} (allowed {allow_b:.3e})")
    assert abs(S[1]) <= allow_a and abs(S[2]) <= allow_b, what


PLANTED = {"softmax": (2.0, 0.0), "bce": (2.0, -1.0)}


@pytest.mark.parametrize("loss", HEADS)
def test_fit_device_on_planted_parameters(loss):
    from euromillioner_amd.ops import calibration_fit as CF

    ta, tb = PLANTED[loss]
    z, tm = SR.planted(loss, a=ta, b=tb)
    masks = torch.from_numpy(np.concatenate([[0], tm])).cuda()  # row s is scored against masks[s + 1]
    fit = CF.fit_device(torch.from_numpy(z).cuda(), masks, len(z), loss)
    assert fit["a"].dtype == np.float32 and max(fit["iterations"]) <= 30
    assert np.all(fit["L_after"] <= fit["L_before"]) and (loss == "bce" or not fit["b"].any())
    S, A = SR.reference(z, SR.bits(tm), loss, fit["a"], fit["b"])
    print(f"{loss}: a {fit['a'].tolist()} b {fit['b'].tolist()}, {fit['iterations']} iterations, {fit['passes']} passes, "
          f"converged {fit['converged']}")
    for g in (0, 1):
        _gradient_vanishes(S[g], A[g], fit["a"][g], fit["b"][g], f"{loss} group {g}")
        assert SR.distance(fit["a"][g], fit["b"][g], ta, tb, S[g]) <= 5.0


# ----------------------------------------------------------------------------------------------- end to end
DATA = ["--n-draws", "3000", "--planted", "0.6", "--seed", "3"]
KINDS = {"mlp": (["--model", "mlp", "--steps", "40", "--batch", "256", "--eval-every", "0", "--loss", "bce"], "m.zip"),
         "counts": (["--model", "counts", "--lags", "2"], "c.cnt")}


def _result(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{") and '"calibration"' in l]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("kind", list(KINDS))
def test_cli_calibrate_on_the_gpu(kind, tmp_path, capsys):
    """``calibrate`` on the GPU against ``--device cpu`` on the same checkpoint, and ``evaluate --calibrator`` against
    the numpy engine on the device's own logits.  The two engines see different logits (bf16 kernels, fast exp), so
    their calibrators are held to the standardised distance 5; the GPU fit is held to the vanishing-gradient rule on
    the logits it saw.  Under bce the reliability tables are equal integer for integer; under softmax an element next
    to an edge may sit one bin across (the slack tests/test_calibration_gpu.py grants em_draw_calibration), so there
    the per-group integers are equal and at most 2 x NEAR_CAP of the elements may move."""
    import _calibration_ref as CR
    from euromillioner_amd import calibration as CAL
    from euromillioner_amd import config as C
    from euromillioner_amd import scaling as SC
    from euromillioner_amd import train as T
    from euromillioner_amd.cli import main

    flags, name = KINDS[kind]
    ck = str(tmp_path / name)
    assert main(["train", "--ckpt", ck] + flags + DATA) == 0
    capsys.readouterr()
    assert main(["calibrate", "--ckpt", ck] + DATA) == 0
    res = _result(capsys.readouterr().out)
    assert res["engine"] == "hip" and res["model"] == kind
    gpu = SC.Calibrator.load(ck + ".cal")
    assert main(["calibrate", "--device", "cpu", "--ckpt", ck, "--out", ck + ".cpu.cal"] + DATA) == 0
    capsys.readouterr()
    cpu = SC.Calibrator.load(ck + ".cpu.cal")
    assert {k: v for k, v in gpu.record.items() if k in ("model", "lags", "first", "last", "rows")} == \
           {k: v for k, v in cpu.record.items() if k in ("model", "lags", "first", "last", "rows")}
    first, last, rows, loss = gpu.record["first"], gpu.record["last"], gpu.record["rows"], gpu.loss
    assert gpu.record["loss_after"] <= gpu.record["loss_before"]

    # the logits the GPU fit saw, on the host
    cfg = C.build_config(None, {"data.n_draws": 3000, "data.planted": 0.6, "data.seed": 3, "ckpt.path": ck})
    s = T._eval_setup(cfg, None, "evaluate")
    assert s.use_gpu and (s.margin, s.loss) == (first, loss)
    z = s.logits_of(s.n - first, first, None)[:, :64].cpu().numpy()
    tm = s.targets[first + 1:s.n + 1].cpu().numpy()
    S, A = SR.reference(z[:rows], SR.bits(tm[:rows]), loss, gpu.a, gpu.b)
    for g in (0, 1):
        _gradient_vanishes(S[g], A[g], gpu.a[g], gpu.b[g], f"{kind} group {g}")
        d = SR.distance(gpu.a[g], gpu.b[g], float(cpu.a[g]), float(cpu.b[g]), S[g])
        print(f"{kind} group {g}: hip a {gpu.a[g]} b {gpu.b[g]}, numpy a {cpu.a[g]} b {cpu.b[g]}, distance {d:.4f}")
        assert d <= 5.0

    assert main(["evaluate", "--ckpt", ck, "--calibrator", ck + ".cal"] + DATA) == 0
    ev = _result(capsys.readouterr().out)
    assert ev["engine"] == "hip" and ev["rows"] == s.n - last and ev["first"] == last
    assert ev["val"] == res["after"]["val"] and ev["calibration"] == res["after"]["calibration"]
    applied = gpu.apply_np(z[rows:])
    spec = CAL.report(CAL.calibration_np(applied, tm[rows:], loss, CAL.DEFAULT_EDGES), s.n - last, loss, CAL.DEFAULT_EDGES)
    for grp in ("main", "stars"):
        got, want = ev["calibration"][grp], spec[grp]
        assert got["count"] == want["count"] and got["hits"] == want["hits"]
        if loss == "bce":
            assert [x["count"] for x in got["bins"]] == [x["count"] for x in want["bins"]], grp
            assert [x["observed"] for x in got["bins"]] == [x["observed"] for x in want["bins"]], grp
        else:
            moved = sum(abs(x["count"] - y["count"]) for x, y in zip(got["bins"], want["bins"]))
            assert moved <= 2 * CR.NEAR_CAP * want["count"], (grp, moved)
