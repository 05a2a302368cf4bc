"""fp64 CPU references and comparison rules for the fused 62->128->62 MLP kernels, the draw-metric kernel
and the loss kernel of the GEMM path (tests/test_fused_ref_cpu.py, test_fused_states_gpu.py,
test_draw_metrics_gpu.py, test_loss_grad_edges_gpu.py).  Nothing in this module touches the GPU.

Parameter states (``make_state``), all as ``state_dict``s of fp32 CPU tensors:

* ``init``    the seed init every older test runs at: Xavier weights, b1 = b2 = 0;
* ``biased``  weights x 3, b1 = 0.5 randn, b2[o] = (0.25 + 0.03 o) (-1)^o: all 62 values distinct and any two
              >= 0.06 apart, so a b2 column read from the wrong place moves a logit by far more than any
              tolerance below;
* ``hot``     weights x 10, the same b1, the ``biased`` b2 + 40 on the 50 main outputs and - 40 on the 12 stars:
              logits span about -126 .. +115, so a softmax maximum shared between the groups underflows every
              star's exp in fp32 and a missing max subtraction overflows.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

LN2 = math.log(2.0)
STATES = ("init", "biased", "hot")
MUTATIONS = ("drop_b1", "b2_logical", "swap_nibbles_13_15")
THR_MARGIN = 1e-3  # |lp + ln 2| below this: the softmax threshold bit of that output is left undecided


def out_phys(o: int) -> int:
    """csrc/mlp_adam.h out_phys: the position of logical output o in the weight images."""
    return o if o < 52 else o + 4 if o < 60 else o - 6 if o < 62 else o - 10


# ---------------------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def draw_masks(n: int = 66000, seed: int = 11) -> torch.Tensor:
    """[n] int64 feature masks of synthetic draws (bit o = output / input o, 5 mains + 2 stars per row)."""
    from euromillioner_amd.data.draws import DrawSet, mask_bits

    ds = DrawSet.synthetic(n=n, seed=seed, planted=0.6, calendar=False)
    return torch.from_numpy(mask_bits(ds.numbers).view("int64").copy())


def bits(masks: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[n] int64 masks -> [n, 62] {0, 1}."""
    return ((masks.cpu()[:, None] >> torch.arange(62)) & 1).to(dtype)


def xy(masks: torch.Tensor, B: int, offset: int = 0, sidx: torch.Tensor | None = None):
    """Inputs and targets of samples offset .. offset + B - 1 (or sidx[:B]): sample i is (draw i, draw i + 1)."""
    idx = sidx[:B].cpu().long() if sidx is not None else torch.arange(offset, offset + B)
    m = masks.cpu()
    return bits(m[idx]), bits(m[idx + 1])


# ---------------------------------------------------------------------------------------------- states
def make_state(name: str, seed: int = 5) -> dict[str, torch.Tensor]:
    from euromillioner_amd.models.mlp import DrawMLP

    if name not in STATES:
        raise ValueError(name)
    ref = DrawMLP((62, 128, 62), seed=seed)
    W1, W2 = ref.layers[0].weight.data.clone(), ref.layers[1].weight.data.clone()
    b1, b2 = torch.zeros(128), torch.zeros(62)
    if name != "init":
        k = 3.0 if name == "biased" else 10.0
        W1, W2 = W1 * k, W2 * k
        b1 = 0.5 * torch.randn(128, generator=torch.Generator().manual_seed(1000 + seed))
        o = torch.arange(62, dtype=torch.float64)
        b2 = (0.25 + 0.03 * o) * (1.0 - 2.0 * (o % 2))
        if name == "hot":
            b2[:50] += 40.0
            b2[50:] -= 40.0
        b2 = b2.float()
    return {"l1.weight": W1, "l1.bias": b1, "l2.weight": W2, "l2.bias": b2}


def _rnd(bf16: bool):
    """The kernels' operand rounding (round to nearest even) in the tensor's own dtype."""
    return (lambda t: t.to(torch.bfloat16).to(t.dtype)) if bf16 else (lambda t: t)


# ---------------------------------------------------------------------------------------------- reference
def ref_forward(sd, X, bf16: bool, dtype=torch.float64, mutation: str | None = None, hidden: bool = False):
    """Logits [B, 62] of the 62->128->62 ReLU MLP.  ``bf16``: W1, b1, W2 and h rounded to bf16, b2 fp32 (the
    bf16 kernels' operands).  ``mutation`` builds a deliberately wrong forward pass (MUTATIONS) for the checks
    of the comparison rules themselves; ``dtype=torch.float32`` evaluates the same formula in fp32."""
    rnd = _rnd(bf16)
    W1, b1, W2 = (rnd(sd[k].to(dtype)) for k in ("l1.weight", "l1.bias", "l2.weight"))
    b2 = sd["l2.bias"].to(dtype)
    X = X.to(dtype)
    if mutation == "drop_b1":  # a forward kernel without BIAS_BIT
        b1 = torch.zeros_like(b1)
    a = X @ W1.t() + b1
    h = rnd(torch.relu(a))
    if mutation == "b2_logical":  # b2 read in logical order by a kernel whose outputs sit in physical order
        b64 = torch.cat([b2, b2.new_zeros(2)])
        b2 = b64[[out_phys(o) for o in range(62)]]
    z = h @ W2.t() + b2
    if mutation == "swap_nibbles_13_15":  # outputs 52-55 and 60-63 trade places on the way out
        z64 = torch.cat([z, z.new_zeros(z.shape[0], 2)], 1)
        idx = list(range(64))
        idx[52:56], idx[60:64] = idx[60:64], idx[52:56]
        z = z64[:, idx][:, :62]
    elif mutation not in (None, "drop_b1", "b2_logical"):
        raise ValueError(mutation)
    return (z, a, h) if hidden else z


def loss_and_dz(z, Y, loss: str, shared_max: bool = False):
    """(per-sample loss [B], dL_sample/dz [B, 62]) written out by hand in z's dtype.  softmax: the grouped
    cross-entropy (50 mains, 12 stars, each against its normalised multi-hot target); bce: mean of 62
    sigmoid cross-entropies.  ``shared_max``: the deliberately wrong softmax whose two groups share one
    maximum."""
    Y = Y.to(z.dtype)
    if loss == "softmax":
        per = z.new_zeros(z.shape[0])
        dz = torch.zeros_like(z)
        for sl in (slice(0, 50), slice(50, 62)):
            zg, yg = z[:, sl], Y[:, sl]
            m = (z if shared_max else zg).max(1, keepdim=True).values
            e = torch.exp(zg - m)
            s = e.sum(1, keepdim=True)
            lp = zg - m - torch.log(s)
            cnt = yg.sum(1, keepdim=True)
            n = cnt.clamp_min(1.0)
            per = per - (yg * lp).sum(1) / n.squeeze(1)
            dz[:, sl] = (e / s * cnt - yg) / n
        return per, dz
    if loss == "bce":
        sp = z.clamp_min(0.0) + torch.log1p(torch.exp(-z.abs()))
        return (sp - Y * z).sum(1) / 62.0, (torch.sigmoid(z) - Y) / 62.0
    raise ValueError(loss)


def ref_loss_grads(sd, X, Y, loss: str, bf16: bool, dtype=torch.float64, shared_max: bool = False,
                   mutation: str | None = None):
    """(mean loss, gradients by state_dict name, logits) of one batch; the backward pass passes straight
    through the bf16 rounding of h, as the kernels' does."""
    rnd = _rnd(bf16)
    z, a, h = ref_forward(sd, X, bf16, dtype, mutation=mutation, hidden=True)
    W2 = rnd(sd["l2.weight"].to(dtype))
    X = X.to(dtype)
    B = X.shape[0]
    per, dz = loss_and_dz(z, Y, loss, shared_max)
    dz = dz / B
    da = (dz @ W2) * (a > 0).to(dtype)
    g = {"l1.weight": da.t() @ X, "l1.bias": da.sum(0), "l2.weight": dz.t() @ h, "l2.bias": dz.sum(0)}
    return float(per.sum() / B), g, z


# ---------------------------------------------------------------------------------------------- logits rule
class LogitRef:
    """fp64 logits of rows 0 .. n - 1 of ``draw_masks()`` at one state, with the two error tiers of the
    logits comparison (check_logits):

    * ``tier``  = 16 x the largest |fp32 - fp64| of the reference formula itself on these rows.  The kernels
      differ from it only in the accumulation order and rounding of their MFMA chains;
    * ``flip``  = 2^-8 sum_c |h_c| |W2_co| per element: what a bf16 rounding of h that falls the other way can
      move a logit by.  Only the bf16 kernel may use it, for at most 0.1 % of the elements."""

    def __init__(self, sd, masks, n: int, bf16: bool):
        X = bits(masks[:n])
        self.bf16 = bf16
        self.z, _, h = ref_forward(sd, X, bf16, hidden=True)
        z32 = ref_forward(sd, X, bf16, dtype=torch.float32).double()
        self.ref_err = float((z32 - self.z).abs().max())
        self.tier = 16.0 * self.ref_err
        W2 = _rnd(bf16)(sd["l2.weight"].double())
        self.flip = 2.0 ** -8 * (h.abs() @ W2.abs().t())

    def rows(self, idx):
        return self.z[idx], self.flip[idx]


def check_logits(got: torch.Tensor, z: torch.Tensor, flip: torch.Tensor, tier: float, allow_flips: bool) -> dict:
    """The logits comparison of tests/test_fused_states_gpu.py; raises AssertionError.  Returns the measured figures."""
    err = (got.double().cpu()[:, :62] - z).abs()
    outside = ~(err <= tier)  # (a NaN is outside)
    n_out = int(outside.sum())
    stats = {"max_err": float(err.max()) if err.numel() else 0.0, "tier": tier, "outside": n_out, "n": err.numel()}
    if not allow_flips:
        assert n_out == 0, stats
        return stats
    assert bool((err[outside] <= flip[outside]).all()), (stats, float((err - flip)[outside].max()))
    assert n_out <= 1e-3 * err.numel(), stats
    return stats


# ---------------------------------------------------------------------------------------------- gradient rule
def grad_tolerances(bf16: bool, B: int) -> tuple[float, float]:
    """(per-tensor relative L2, loss) tolerances of the project's existing gradient tests."""
    if bf16:
        return (1e-2 if B >= 256 else 3e-2), 2e-3
    return 3e-5, 3e-5


def grad_errors(gk_flat: torch.Tensor, gref: dict) -> dict[str, float]:
    from euromillioner_amd.ops import fused_mlp as FM

    got = FM.unflatten(gk_flat.double().cpu())
    out = {}
    for name in ("l1.weight", "l1.bias", "l2.weight", "l2.bias"):
        r = gref[name].double()
        out[name] = float((got[name] - r).norm() / r.norm().clamp_min(1e-300))
    return out


def check_grads(lk: float, gk_flat: torch.Tensor, lref: float, gref: dict, bf16: bool, B: int, tol=None) -> dict:
    """The gradient and loss comparison of tests/test_fused_states_gpu.py; raises AssertionError."""
    from euromillioner_amd.ops import fused_mlp as FM

    gtol, ltol = grad_tolerances(bf16, B)
    if tol is not None:
        gtol = tol
    errs = grad_errors(gk_flat, gref)
    stats = {"loss": lk, "loss_ref": lref, "errs": errs, "tol": gtol}
    assert abs(lk - lref) <= ltol * max(1.0, abs(lref)), stats  # (fails on a NaN / inf loss)
    for name, e in errs.items():
        assert e <= gtol, (name, stats)
    assert float((gk_flat.cpu() * (1 - FM.pad_mask())).abs().max()) == 0.0, "padding slots must stay exactly 0"
    return stats


def flat_grads(g: dict) -> torch.Tensor:
    """Reference-shaped gradients -> the kernels' flat fp32 layout (for the mutation checks)."""
    from euromillioner_amd.ops import fused_mlp as FM

    return FM.flatten({k: v.float() for k, v in g.items()})


# ---------------------------------------------------------------------------------------------- logit families
FAMILIES = ("randn3", "signal", "integers", "randn80", "spikes")
SIGNAL_A = 4.0  # "signal": a Y + randn; a = 12 predicts every draw exactly, this leaves exact inside (0.05, 0.95)


def logit_family(name: str, Y: torch.Tensor, seed: int = 0) -> torch.Tensor:
    """[B, 64] fp32 logits (pads 0) for targets Y [B, 62]."""
    B = Y.shape[0]
    g = torch.Generator().manual_seed(100 + seed)
    r = torch.randn(B, 62, generator=g, dtype=torch.float64)
    if name == "randn3":
        z = 3.0 * r
    elif name == "signal":
        z = SIGNAL_A * Y.double() + r
    elif name == "integers":  # ties across the top-5 / top-2 boundary in nearly every row
        z = torch.randint(-2, 3, (B, 62), generator=g).double()
    elif name == "randn80":
        z = 80.0 * r
    elif name == "spikes":  # one main and one star far above the rest: softmax threshold bits get set
        z = r.clone()
        rows = torch.arange(B)
        z[rows, torch.randint(0, 50, (B,), generator=g)] += 15.0
        z[rows, 50 + torch.randint(0, 12, (B,), generator=g)] += 15.0
    elif name == "groups40":  # the hot state's group offsets
        z = 3.0 * r
        z[:, :50] += 40.0
        z[:, 50:] -= 40.0
    else:
        raise ValueError(name)
    out = torch.zeros(B, 64, dtype=torch.float32)
    out[:, :62] = z.float()
    return out


def log_probs(z: np.ndarray) -> np.ndarray:
    """fp64 grouped log-softmax of [B, 62] logits."""
    def lsm(a):
        m = a.max(1, keepdims=True)
        return a - m - np.log(np.exp(a - m).sum(1, keepdims=True))

    z = np.asarray(z, dtype=np.float64)
    return np.concatenate([lsm(z[:, :50]), lsm(z[:, 50:62])], axis=1)


def near_threshold(z: np.ndarray, loss: str) -> np.ndarray:
    """[B, 62] bool: outputs whose softmax threshold bit (lp >= -ln 2, computed by the kernel with fast exp /
    log) is left undecided: fp64 lp within THR_MARGIN of -ln 2.  bce thresholds z >= 0 on the same fp32
    numbers as the reference, so nothing is undecided there."""
    z = np.asarray(z, dtype=np.float64)[:, :62]
    if loss != "softmax":
        return np.zeros(z.shape, dtype=bool)
    return np.abs(log_probs(z) + LN2) < THR_MARGIN


COUNT_METRICS = ("hits_main", "hits_star", "exact", "count")
MEAN_TOL = 256 * 2.0 ** -23  # acc / acc_thr / trivial_acc: 256 fp32 terms of one block
LOSS_TOL = 1e-4  # the project's figure for the sister kernel (tests/test_gemm_gpu.py test_loss_grad_kernel)


def metric_sums(z: torch.Tensor, Y: torch.Tensor, loss: str) -> dict[str, float]:
    """Sums over the rows of z of euromillioner_amd.metrics.draw_metrics (fp64 numpy, stable argsort: the
    earlier index wins a tie); count-valued metrics come back as exact integers.  ``slack`` = the number of
    undecided threshold bits / 62: how far acc_thr may move."""
    from euromillioner_amd.metrics import draw_metrics

    zn, yn = z.double().numpy()[:, :62], Y.numpy()
    n = len(zn)
    ref = draw_metrics(zn, yn, loss)
    out = {}
    for k, v in ref.items():
        s = v * n if k != "count" else float(v)
        if k in COUNT_METRICS:
            assert abs(s - round(s)) < 1e-6, (k, s)
            s = float(round(s))
        out[k] = s
    near = near_threshold(zn, loss)
    out["slack"] = float(near.sum()) / 62.0
    out["near_rows"] = int(near.any(1).sum())
    return out


def check_metric_sums(got: dict[str, float], ref: dict[str, float], rel_scale: float = 1.0) -> None:
    """The per-block comparison of tests/test_draw_metrics_gpu.py.  ``got`` / ``ref``: sums over the same rows."""
    for k in COUNT_METRICS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("acc", "trivial_acc"):
        assert abs(got[k] - ref[k]) <= MEAN_TOL * rel_scale * abs(ref[k]), (k, got[k], ref[k])
    assert abs(got["acc_thr"] - ref["acc_thr"]) <= MEAN_TOL * rel_scale * abs(ref["acc_thr"]) + ref["slack"], \
        ("acc_thr", got["acc_thr"], ref["acc_thr"], ref["slack"])
    assert abs(got["loss"] - ref["loss"]) <= LOSS_TOL * abs(ref["loss"]), ("loss", got["loss"], ref["loss"])
