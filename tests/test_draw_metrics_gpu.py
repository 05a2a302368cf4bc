"""em_draw_metrics per 256-row block, and the evaluate() loops built on it, against the fp64 numpy reference
euromillioner_amd.metrics.draw_metrics (stable argsort: the earlier index wins a tie) fed the SAME fp32 logits.

Per block: hits_main, hits_star, exact and count are equal as integers; acc, acc_thr and trivial_acc agree within
256 x 2^-23 relative (256 fp32 terms); the loss within 1e-4 relative (the project's figure for the sister loss
kernel).  acc_thr under softmax compares lp with -ln 2 after a fast exp / log: an output whose fp64 lp lies within
1e-3 of -ln 2 (_fused_ref.THR_MARGIN) is left undecided, i.e. the block's acc_thr sum may move by 1/62 per such
output, and at most 2 % of the rows may hold one (CPU check, B = 1301: 0.3 % for 3 randn and a Y + randn, none for
the other three families; tests/test_fused_ref_cpu.py asserts it).

The ``integers`` family (logits in {-2 .. 2}: ties across the top-5 / top-2 boundary in ~99 % of the rows) is the
one that caught topk_mask dropping the EARLIER of two equal entries when a larger value was inserted above them
(about 1 % of such rows picked a different main number); the kernel now shifts displaced entries unconditionally."""
import numpy as np
import pytest
import torch

import _fused_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def draws():
    return R.draw_masks().cuda()


def _block_sums(part: torch.Tensor) -> list[dict[str, float]]:
    from euromillioner_amd.ops.fused_mlp import METRIC_NAMES

    p = part.double().cpu().numpy()
    return [dict(zip(METRIC_NAMES, row)) for row in p]


def _check_blocks(part, z, Y, loss, what):
    B = z.shape[0]
    blocks = _block_sums(part)
    assert len(blocks) == (B + 255) // 256
    near = 0
    for b, got in enumerate(blocks):
        sl = slice(256 * b, min(256 * (b + 1), B))
        ref = R.metric_sums(z[sl], Y[sl], loss)
        near += ref["near_rows"]
        try:
            R.check_metric_sums(got, ref)
        except AssertionError as e:
            raise AssertionError(f"{what} block {b}: {e}") from e
    return near


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("loss", ["softmax", "bce"])
def test_draw_metrics_blocks_match_numpy(draws, loss, family):
    from euromillioner_amd.ops import fused_mlp as FM

    masks = R.draw_masks()
    near = rows = 0
    for B in (1, 255, 256, 257, 1301):
        for off in (0, 17):
            _, Y = R.xy(masks, B, off)
            z = R.logit_family(family, Y, seed=B + off)
            part = FM.draw_metrics(z.cuda(), draws, B, loss=loss, offset=off)
            near += _check_blocks(part, z, Y, loss, f"{family} {loss} B={B} offset={off}")
            rows += B
    # once through a shuffled sample index with repeats
    B = 1301
    sidx = torch.randint(0, 5000, (B,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    sidx[250:262] = sidx[0]
    _, Y = R.xy(masks, B, sidx=sidx)
    z = R.logit_family(family, Y, seed=77)
    part = FM.draw_metrics(z.cuda(), draws, B, loss=loss, sidx=sidx.cuda())
    near += _check_blocks(part, z, Y, loss, f"{family} {loss} B={B} sidx")
    rows += B
    print(f"{family} {loss}: {near} of {rows} rows hold an undecided threshold bit")
    assert near <= 0.02 * rows


def _gemm_state(seed=4):
    """(62, 96, 62) at biased-style parameters: weights x 3, b1 = 0.5 randn, the ``biased`` b2."""
    from euromillioner_amd.models.mlp import DrawMLP

    sd = {k: v.clone() for k, v in DrawMLP((62, 96, 62), seed=seed).state_dict().items()}
    sd["layers.0.weight"] *= 3.0
    sd["layers.1.weight"] *= 3.0
    sd["layers.0.bias"] = 0.5 * torch.randn(96, generator=torch.Generator().manual_seed(seed))
    sd["layers.1.bias"] = R.make_state("biased")["l2.bias"].clone()
    return sd


def _make(kind, loss):
    if kind == "gemm":
        from euromillioner_amd.models.gemm_mlp import GemmMLPTrainer

        return GemmMLPTrainer((62, 96, 62), loss=loss, state_dict=_gemm_state())
    from euromillioner_amd.models.mlp import FusedSmallMLP

    return FusedSmallMLP(loss=loss, state_dict=R.make_state("biased"), dtype=kind)


@pytest.mark.parametrize("kind", ["bf16", "fp32", "gemm"])
@pytest.mark.parametrize("loss", ["softmax", "bce"])
def test_evaluate_chunks_and_sample_index(draws, loss, kind):
    """evaluate() at non-zero biases, B = 1301 from offset 5: in chunks of 500, in one chunk and through an
    identity sample index.  Count-valued metrics are identical across the three, the others agree within 1e-6,
    and all match the numpy reference applied to the model's own logits()."""
    m = _make(kind, loss)
    B, off = 1301, 5
    ident = torch.arange(off, off + B, dtype=torch.int32, device="cuda")
    runs = {"chunk=500": m.evaluate(draws, B, offset=off, chunk=500), "default": m.evaluate(draws, B, offset=off),
            "sidx": m.evaluate(draws, B, sidx=ident)}
    base = runs["default"]
    for name, ev in runs.items():
        print(f"{kind} {loss} {name}: {ev}")
        assert ev["count"] == B
        for k in ("hits_main", "hits_star", "exact"):
            assert ev[k] == base[k], (name, k, ev[k], base[k])
        for k in ("loss", "acc", "acc_thr", "trivial_acc"):
            assert abs(ev[k] - base[k]) <= 1e-6 * max(1.0, abs(base[k])), (name, k, ev[k], base[k])
    z = m.logits(draws, B, offset=off).clone().cpu()
    assert z.shape == (B, 64)
    _, Y = R.xy(R.draw_masks(), B, off)
    ref = R.metric_sums(z, Y, loss)
    assert ref["near_rows"] <= 0.02 * B
    for name, ev in runs.items():
        got = {k: ev[k] * B for k in ("loss", "acc", "acc_thr", "trivial_acc")}
        for k in ("hits_main", "hits_star", "exact"):
            s = ev[k] * B
            assert abs(s - round(s)) < 1e-6, (k, s)
            got[k] = float(round(s))
        got["count"] = float(ev["count"])
        try:
            R.check_metric_sums(got, ref)
        except AssertionError as e:
            raise AssertionError(f"{kind} {loss} {name}: {e}") from e
    assert 0.0 < np.float64(ref["acc"]) / B < 1.0
