"""The fused forward kernel and both fused train kernels against the fp64 reference of tests/_fused_ref.py at
three parameter states: the seed init, ``biased`` (non-zero b1 and 62 distinct b2 values: the b1 row behind
BIAS_BIT, the b2 read through the out_phys permutation and pack_one's b2 branch carry data) and ``hot``
(logits -126 .. +115, main and star groups 80 apart: the softmax's per-group maxima matter).

Logit tolerance (check_logits): tight tier = 16 x the largest |fp32 - fp64| of the reference formula on the same
rows, computed in the test (CPU fp32 vs fp64, rows 0 .. 4096: init 1.2e-7 -> 1.9e-6, biased 1.4e-6 -> 2.2e-5,
hot 1.4e-5 -> 2.2e-4 for the bf16 operands; fp32 operands 3.6e-7 / 3.1e-6 / 3.2e-5 -> 5.7e-6 / 5.0e-5 / 5.2e-4).
The bf16 kernel may leave the tier for at most 0.1 % of the elements, each within 2^-8 sum_c |h_c| |W2_co| (an h
that rounds to the other bf16 neighbour); the fp32 path may not leave it at all.

Measured on an MI355X: the bf16 forward kernel's largest error is 1.5e-7 (init), 1.9e-6 (biased) and 2.6e-5 (hot),
the fp32 path's 4.4e-7 / 3.9e-6 / 3.5e-5, i.e. about the reference's own fp32 error; no element left the tier.

Gradient tolerances are the project's (per-tensor relative L2 1e-2, 3e-2 below 256 rows, fp32 3e-5; loss 2e-3 /
3e-5), unchanged at ``hot``: measured there at most 5.7e-4 (bf16, 1100 rows), 1.5e-3 (bf16, 37 rows) and 9.3e-7
(fp32)."""
import functools

import pytest
import torch

import _fused_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
DTYPES = ("bf16", "fp32")


@pytest.fixture(scope="module")
def draws():
    return R.draw_masks().cuda()


@functools.lru_cache(maxsize=None)
def _sd(state):
    return R.make_state(state)


@functools.lru_cache(maxsize=None)
def _logit_ref(state, bf16, n=4097):
    return R.LogitRef(_sd(state), R.draw_masks(), n, bf16)


_models = {}


def _model(state, dtype, loss="softmax"):
    """One model per (state, dtype, loss), shared by the tests that do not train it."""
    from euromillioner_amd.models.mlp import FusedSmallMLP

    key = (state, dtype, loss)
    if key not in _models:
        _models[key] = FusedSmallMLP(loss=loss, state_dict=_sd(state), dtype=dtype)
    return _models[key]


def _logits(m, draws, B, offset=0, sidx=None, extra_rows=0):
    """m.logits; the bf16 forward kernel writes into a caller-supplied buffer with ``extra_rows`` sentinel rows."""
    if m.dtype == "fp32":
        return m.logits(draws, B, offset=offset, sidx=sidx)
    out = torch.full((B + extra_rows, 64), SENTINEL, dtype=torch.float32, device="cuda")
    res = m.FM.forward_logits(draws, B, m.img, out=out, offset=offset, sidx=sidx)
    assert res.data_ptr() == out.data_ptr()
    return out


def _check(lg, B, ref, idx, bf16, what):
    assert float(lg[:B, 62:].abs().max()) == 0.0, f"{what}: pad outputs must read exactly 0"
    if lg.shape[0] > B:
        assert bool((lg[B:] == SENTINEL).all()), f"{what}: rows >= B were written"
    z, flip = ref.rows(idx)
    stats = R.check_logits(lg[:B], z, flip, ref.tier, allow_flips=bf16)
    print(f"  {what}: max |err| {stats['max_err']:.2e} tier {stats['tier']:.2e} outside {stats['outside']}/{stats['n']}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("state", R.STATES)
def test_logits_match_fp64_reference(draws, state, dtype):
    """B around the 32-row tile and the 128-row workgroup, a single row, several workgroups; offsets 0 and 7."""
    bf16 = dtype == "bf16"
    m, ref = _model(state, dtype), _logit_ref(state, bf16)
    for B in (1, 31, 32, 33, 127, 128, 129, 3001):
        for off in (0, 7):
            lg = _logits(m, draws, B, offset=off, extra_rows=3)
            _check(lg, B, ref, torch.arange(off, off + B), bf16, f"{state} {dtype} B={B} offset={off}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("state", R.STATES)
def test_logits_grid_stride(draws, state, dtype):
    """2 x CUs x 128 + 33 rows: the forward kernel's grid is capped at 2 workgroups per CU, so every wave loops."""
    from euromillioner_amd.ops import _native as N

    bf16 = dtype == "bf16"
    B = 2 * N.cu_count(draws.device) * 128 + 33
    assert B + 1 <= draws.shape[0]
    m, ref = _model(state, dtype), _logit_ref(state, bf16, B)
    lg = _logits(m, draws, B, extra_rows=2)
    _check(lg, B, ref, torch.arange(B), bf16, f"{state} {dtype} B={B}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("state", ["biased", "hot"])
def test_logits_through_sample_index(draws, state, dtype):
    """sidx: the identity index is bit-equal to the offset path; a shuffled index with repeats matches the
    reference row by row."""
    bf16 = dtype == "bf16"
    m, ref = _model(state, dtype), _logit_ref(state, bf16)
    B, off = 1001, 7
    ident = torch.arange(off, off + B, dtype=torch.int32, device="cuda")
    assert torch.equal(_logits(m, draws, B, sidx=ident), _logits(m, draws, B, offset=off))
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 4097, (B,), generator=g, dtype=torch.int32)
    idx[5:40] = idx[4]  # a run of repeats across a tile edge
    assert idx.unique().numel() < B
    lg = _logits(m, draws, B, sidx=idx.cuda(), extra_rows=1)
    _check(lg, B, ref, idx.long(), bf16, f"{state} {dtype} shuffled sidx")


def _grads_on_slabs(m, draws, B, offset, nrows):
    """grads() on an ``nrows``-row slab tensor (tests/test_fused_issue_diet_gpu.py: two workgroups wrap the ring)."""
    FM = m.FM
    slabs = torch.zeros(nrows, FM.SLAB_STRIDE, dtype=torch.float32, device="cuda")
    loss_slabs = torch.zeros(nrows, dtype=torch.float32, device="cuda")
    if m.dtype == "fp32":
        nslab = FM.train_partials_f32(draws, B, m.params, slabs, loss_slabs, loss=m.loss_name, offset=offset)
    else:
        nslab = FM.train_partials(draws, B, m.img, slabs, loss_slabs, loss=m.loss_name, offset=offset)
    assert nslab == nrows
    scale = 1.0 / B / (62.0 if m.loss_name == "bce" else 1.0)
    FM.adam_slab(slabs, nslab, scale, m.params, m.m, m.v, m.hp, m.state, mode=1, grad_io=m.grad_io,
                 loss_slabs=loss_slabs, loss_out=m.grad_io[FM.P_TOTAL:], loss_scale=scale)
    return m.grad_io[FM.P_TOTAL].item(), m.grad_io[:FM.P_TOTAL].clone()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loss", ["softmax", "bce"])
@pytest.mark.parametrize("state", ["biased", "hot"])
def test_grads_match_fp64_reference(draws, state, loss, dtype):
    """grads() of both train kernels: a partial tile (B = 37), 35 tiles (B = 1100) on the default grid and on two
    workgroups, and a shuffled sample index with repeats at a partial tile (B = 45)."""
    bf16 = dtype == "bf16"
    m, sd, masks = _model(state, dtype, loss), _sd(state), R.draw_masks()
    g = torch.Generator().manual_seed(9)
    sidx = torch.randint(0, 4000, (45,), generator=g, dtype=torch.int32)
    sidx[30:36] = sidx[2]
    cases = [("B=37", 37, 100, None, None), ("B=1100", 1100, 3, None, None), ("B=1100 on 2 workgroups", 1100, 3, None, 2),
             ("B=45 sidx", 45, 0, sidx, None)]
    for what, B, off, si, nrows in cases:
        X, Y = R.xy(masks, B, off, si)
        lref, gref, _ = R.ref_loss_grads(sd, X, Y, loss, bf16)
        if nrows:
            lk, gk = _grads_on_slabs(m, draws, B, off, nrows)
        else:
            lk, gk = m.grads(draws, B, offset=off, sidx=si.cuda() if si is not None else None)
        assert bool(torch.isfinite(gk).all()), what
        stats = R.check_grads(lk, gk, lref, gref, bf16, B)
        errs = " ".join(f"{k}={e:.2e}" for k, e in stats["errs"].items())
        print(f"  {state} {loss} {dtype} {what}: loss {lk!r} ref {lref!r}; {errs} (tol {stats['tol']})")


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_image_follows_adam(draws, dtype):
    """After three optimizer steps from ``biased`` the image Adam wrote is pack(params) byte for byte, and the
    logits read from it match the reference of the model's own state_dict()."""
    from euromillioner_amd.models.mlp import FusedSmallMLP
    from euromillioner_amd.ops import fused_mlp as FM

    bf16 = dtype == "bf16"
    m = FusedSmallMLP(loss="softmax", state_dict=_sd("biased"), dtype=dtype, lr=1e-2)
    img0 = m.img.clone()
    for it in range(3):
        m.step(draws, 2048, offset=100 * it)
    torch.cuda.synchronize()
    assert not torch.equal(m.img, img0)
    fresh = torch.zeros(FM.IMG_BYTES, dtype=torch.uint8, device="cuda")
    FM.pack(m.params, fresh)
    assert torch.equal(fresh, m.img)
    sd = m.state_dict()
    assert float((sd["l2.bias"] - _sd("biased")["l2.bias"]).abs().mean()) > 1e-3  # b2 moved with the rest
    B, off = 3001, 7
    ref = R.LogitRef(sd, R.draw_masks(), off + B, bf16)
    _check(_logits(m, draws, B, offset=off), B, ref, torch.arange(off, off + B), bf16, f"{dtype} after 3 steps")
