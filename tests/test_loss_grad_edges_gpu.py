"""em_loss_grad / em_loss_grad_f32 (the GEMM path's loss kernel: 4 samples per wave, 16 per block, at most 4096
blocks) at its edges, against the by-hand fp64 loss and gradient of tests/_fused_ref.py on the same fp32 logits:
B around the 4-sample wave group and the 16-sample block, one grid-stride batch (65 541 rows on the 4096-block
cap), logits 3 randn, 80 randn (exp underflows inside a group) and +-40 group offsets (a maximum shared between
the groups would underflow every star), and a shuffled sample index with repeats.

dz: relative L2 1e-2 for the bf16 variant (tests/test_gemm_gpu.py test_loss_grad_kernel) and 1e-4 for fp32 (the
fp32 trainer's gradient tolerance, tests/test_gemm_f32_gpu.py); pads exactly 0; the loss partials sum within 1e-4;
each colpart row within 1e-6 of the column's absolute sum of the RETURNED dz of that block's samples."""
import pytest
import torch

import _fused_ref as R

pytestmark = pytest.mark.gpu

LOGIT_FAMILIES = ("randn3", "randn80", "groups40")


@pytest.fixture(scope="module")
def draws():
    return R.draw_masks().cuda()


def _run(variant, z, draws, B, loss, offset=0, sidx=None):
    from euromillioner_amd.ops import linear as LIN
    from euromillioner_amd.ops import linear_f32 as LF

    nb = LIN.loss_grad_blocks(B)
    assert nb == min((B + 15) // 16, 4096)
    colpart = torch.full((nb * 64,), float("nan"), dtype=torch.float32, device="cuda")
    mod = LIN if variant == "bf16" else LF
    dz, part = mod.loss_grad(z, draws, B, loss, offset=offset, sidx=sidx, grad_scale=1.0 / B, colpart=colpart)
    assert dz.dtype == (torch.bfloat16 if variant == "bf16" else torch.float32) and dz.shape == (B, 64)
    assert part.numel() >= (B + 3) // 4
    return dz.double().cpu(), part[:(B + 3) // 4].double().cpu(), colpart.view(nb, 64).double().cpu()


def _check(variant, zc, Y, loss, dz, part, colpart, what):
    B = zc.shape[0]
    per, dref = R.loss_and_dz(zc[:, :62].double(), Y, loss)
    dref = dref / B
    lref = float(per.sum() / B)
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(part).all()), what
    err = float((dz[:, :62] - dref).norm() / dref.norm())
    tol = 1e-2 if variant == "bf16" else 1e-4
    lk = float(part.sum()) / B
    print(f"  {what}: dz relative L2 {err:.2e} (tol {tol}); loss {lk!r} ref {lref!r}")
    assert err <= tol, (what, err)
    assert float(dz[:, 62:].abs().max()) == 0.0, what
    assert abs(lk - lref) <= 1e-4 * max(1.0, abs(lref)), (what, lk, lref)
    # block of sample s: wave group s // 4 runs on global wave (s // 4) % (4 nb), four waves per block
    nb = colpart.shape[0]
    blk = ((torch.arange(B) // 4) % (4 * nb)) // 4
    csum = torch.zeros(nb, 64, dtype=torch.float64).index_add_(0, blk, dz)
    cabs = torch.zeros(nb, 64, dtype=torch.float64).index_add_(0, blk, dz.abs())
    assert bool(((colpart - csum).abs() <= 1e-6 * cabs).all()), (what, float(((colpart - csum).abs() - 1e-6 * cabs).max()))


@pytest.mark.parametrize("variant", ["bf16", "fp32"])
@pytest.mark.parametrize("loss", ["softmax", "bce"])
def test_loss_grad_edges(draws, loss, variant):
    masks = R.draw_masks()
    for B in (1, 3, 4, 5, 15, 16, 17, 1001, 65541):
        off = 17 if B == 1001 else 0
        _, Y = R.xy(masks, B, off)
        for fam in LOGIT_FAMILIES:
            zc = R.logit_family(fam, Y, seed=B)
            dz, part, colpart = _run(variant, zc.cuda(), draws, B, loss, offset=off)
            _check(variant, zc, Y, loss, dz, part, colpart, f"{variant} {loss} {fam} B={B}")


@pytest.mark.parametrize("variant", ["bf16", "fp32"])
@pytest.mark.parametrize("loss", ["softmax", "bce"])
def test_loss_grad_through_sample_index(draws, loss, variant):
    masks = R.draw_masks()
    B = 1001
    sidx = torch.randint(0, 5000, (B,), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    sidx[14:19] = sidx[0]
    _, Y = R.xy(masks, B, sidx=sidx)
    zc = R.logit_family("groups40", Y, seed=1)
    dz, part, colpart = _run(variant, zc.cuda(), draws, B, loss, sidx=sidx.cuda())
    _check(variant, zc, Y, loss, dz, part, colpart, f"{variant} {loss} groups40 B={B} sidx")
