"""CPU self-checks of tests/_fused_ref.py: the fp64 reference, the three parameter states, the logit families
of the metric tests, and mutation checks of the comparison rules the GPU tests apply (a forward pass without
b1, with b2 in logical order, with nibbles 13 / 15 swapped, and a softmax with one shared maximum must each
fail them)."""
import numpy as np
import pytest
import torch

import _fused_ref as R

B_HOT = 1100


@pytest.fixture(scope="module")
def masks():
    return R.draw_masks()


def test_by_hand_gradients_match_autograd(masks):
    """ref_loss_grads (losses and backward pass written out) against torch autograd in fp64."""
    sd = R.make_state("biased")
    X, Y = R.xy(masks, 300, 7)
    for loss in ("softmax", "bce"):
        for bf16 in (True, False):
            l, g, z = R.ref_loss_grads(sd, X, Y, loss, bf16)
            rnd = R._rnd(bf16)
            p = {k: rnd(sd[k].double()).requires_grad_() for k in ("l1.weight", "l1.bias", "l2.weight")}
            b2 = sd["l2.bias"].double().requires_grad_()
            h = torch.relu(X @ p["l1.weight"].t() + p["l1.bias"])
            h = h + (rnd(h) - h).detach()  # straight-through, as the kernel's backward sees it
            za = h @ p["l2.weight"].t() + b2
            if loss == "softmax":
                lm, ls = torch.log_softmax(za[:, :50], 1), torch.log_softmax(za[:, 50:], 1)
                la = (-(Y[:, :50] * lm).sum(1) / 5 - (Y[:, 50:] * ls).sum(1) / 2).mean()
            else:
                la = torch.nn.functional.binary_cross_entropy_with_logits(za, Y)
            la.backward()
            assert torch.equal(za.detach(), z)
            assert abs(l - la.item()) < 1e-12 * max(1.0, abs(l))
            for k, ref in (("l1.weight", p["l1.weight"].grad), ("l1.bias", p["l1.bias"].grad),
                           ("l2.weight", p["l2.weight"].grad), ("l2.bias", b2.grad)):
                assert float((g[k] - ref).norm() / ref.norm()) < 1e-12, (loss, bf16, k)


def test_biased_b2_values_are_distinct():
    b2 = R.make_state("biased")["l2.bias"].double()
    d = (b2[:, None] - b2[None, :]).abs() + 10.0 * torch.eye(62)
    assert float(d.min()) >= 0.06 - 1e-6
    assert float(R.make_state("biased")["l1.bias"].abs().min()) > 0.0
    for name in ("biased", "hot"):
        assert float(R.make_state(name)["l1.bias"].abs().mean()) > 0.2
    assert float(R.make_state("init")["l2.bias"].abs().max()) == 0.0


@pytest.mark.parametrize("bf16", [True, False])
def test_hot_state_facts(masks, bf16):
    """The ``hot`` state at B = 1100: logits about -126 .. +115 with group means +39 / -39, a finite fp64 loss
    and gradient for both losses, and an fp32 evaluation of the same formulas within 1e-6 relative per tensor
    of the fp64 one (measured with torch's CPU fp32 matmuls: at most 5.2e-7, l2.weight under bce), 30 times
    below the 3e-5 the fp32 kernels are held to: the project's tolerances stand at this state."""
    sd = R.make_state("hot")
    X, Y = R.xy(masks, B_HOT, 0)
    z = R.ref_forward(sd, X, bf16)
    print(f"hot logits: min {float(z.min()):.1f} max {float(z.max()):.1f} main mean {float(z[:, :50].mean()):.1f} "
          f"star mean {float(z[:, 50:].mean()):.1f}")
    assert -150.0 < float(z.min()) < -110.0 and 105.0 < float(z.max()) < 145.0
    assert abs(float(z[:, :50].mean()) - 40.0) < 4.0 and abs(float(z[:, 50:].mean()) + 40.0) < 4.0
    for loss in ("softmax", "bce"):
        l64, g64, _ = R.ref_loss_grads(sd, X, Y, loss, bf16)
        l32, g32, _ = R.ref_loss_grads(sd, X, Y, loss, bf16, dtype=torch.float32)
        assert np.isfinite(l64) and all(bool(torch.isfinite(t).all()) for t in g64.values())
        assert np.isfinite(l32) and all(bool(torch.isfinite(t).all()) for t in g32.values())
        assert abs(l32 - l64) <= 1e-6 * abs(l64), (loss, l32, l64)
        for k in g64:
            e = float((g32[k].double() - g64[k]).norm() / g64[k].norm())
            print(f"hot {loss} bf16={bf16} {k}: fp32 vs fp64 {e:.2e}")
            assert e <= 1e-6, (loss, k, e)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("state", ["biased", "hot"])
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_logit_rule_rejects_mutated_forward(masks, state, bf16, mutation):
    """The logits comparison of the GPU tests (tight tier + bf16 flip bound, <= 0.1 % flips) accepts the fp32
    evaluation of the reference and rejects each mutated forward pass, at a full batch and at one row."""
    sd = R.make_state(state)
    ref = R.LogitRef(sd, masks, 4097, bf16)
    for B, off in ((4097, 0), (1, 7)):
        idx = torch.arange(off, off + B)
        z, flip = ref.rows(idx)
        X = R.bits(masks[idx])
        R.check_logits(R.ref_forward(sd, X, bf16, dtype=torch.float32), z, flip, ref.tier, allow_flips=False)
        with pytest.raises(AssertionError):
            R.check_logits(R.ref_forward(sd, X, bf16, mutation=mutation), z, flip, ref.tier, allow_flips=bf16)


def test_logit_tier_is_tight(masks):
    """The tight tier is orders below the 2e-2 of the older forward test: 16 x the reference's own fp32 error."""
    for state in R.STATES:
        for bf16 in (True, False):
            ref = R.LogitRef(R.make_state(state), masks, 4097, bf16)
            print(f"{state} bf16={bf16}: max |fp32 - fp64| {ref.ref_err:.2e} -> tier {ref.tier:.2e}, "
                  f"median flip bound {float(ref.flip.median()):.2e}")
            assert 0.0 < ref.tier < 1e-3
            assert float(ref.flip.min()) >= 0.0


def test_init_state_hides_the_bias_mutations(masks):
    """Why the states exist: at the seed init (b1 = b2 = 0) a forward pass without b1 or with b2 in the wrong
    order is indistinguishable from the correct one."""
    sd = R.make_state("init")
    X = R.bits(masks[:257])
    z = R.ref_forward(sd, X, True)
    for mutation in ("drop_b1", "b2_logical"):
        assert torch.equal(R.ref_forward(sd, X, True, mutation=mutation), z)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("loss", ["softmax", "bce"])
def test_grad_rule_rejects_mutations(masks, loss, bf16):
    """The gradient comparison accepts the fp32 evaluation of the reference, and rejects the mutated forward
    passes and (softmax, ``hot``) a group maximum shared between mains and stars, whose fp32 loss is not finite."""
    B = 1100
    X, Y = R.xy(masks, B, 3)
    for state in ("biased", "hot"):
        sd = R.make_state(state)
        lref, gref, _ = R.ref_loss_grads(sd, X, Y, loss, bf16)
        l32, g32, _ = R.ref_loss_grads(sd, X, Y, loss, bf16, dtype=torch.float32)
        R.check_grads(l32, R.flat_grads(g32), lref, gref, bf16, B)
        for mutation in R.MUTATIONS:
            lm, gm, _ = R.ref_loss_grads(sd, X, Y, loss, bf16, dtype=torch.float32, mutation=mutation)
            with pytest.raises(AssertionError):
                R.check_grads(lm, R.flat_grads(gm), lref, gref, bf16, B)
    if loss == "softmax":
        ls, gs, _ = R.ref_loss_grads(sd, X, Y, loss, bf16, dtype=torch.float32, shared_max=True)
        assert not np.isfinite(ls)
        with pytest.raises(AssertionError):
            R.check_grads(ls, R.flat_grads(gs), lref, gref, bf16, B)
        # (in fp64 the shared maximum is harmless: exp(-165) is a normal number there)
        l64, _, _ = R.ref_loss_grads(sd, X, Y, loss, bf16, shared_max=True)
        assert abs(l64 - lref) < 1e-9 * abs(lref)


def test_grad_rule_rejects_a_dropped_pad_invariant(masks):
    X, Y = R.xy(masks, 300, 0)
    sd = R.make_state("biased")
    lref, gref, _ = R.ref_loss_grads(sd, X, Y, "softmax", False)
    g = R.flat_grads(gref)
    R.check_grads(lref, g, lref, gref, False, 300)
    g[-1] = 1e-20  # b2 pad slot 63
    with pytest.raises(AssertionError):
        R.check_grads(lref, g, lref, gref, False, 300)


@pytest.mark.parametrize("loss", ["softmax", "bce"])
def test_logit_family_conditions(masks, loss):
    """What the metric tests rely on (B = 1301): ``signal`` has exact strictly between 0.05 and 0.95, ``integers``
    ties across the top-5 / top-2 boundary in >= 95 % of the rows, ``spikes`` sets softmax threshold bits, and at
    most 2 % of the rows of any family have a threshold bit within THR_MARGIN of its decision."""
    from euromillioner_amd.metrics import draw_metrics

    B = 1301
    _, Y = R.xy(masks, B, 0)
    for fam in R.FAMILIES:
        z = R.logit_family(fam, Y)
        assert z.dtype == torch.float32 and z.shape == (B, 64) and float(z[:, 62:].abs().max()) == 0.0
        ref = R.metric_sums(z, Y, loss)
        print(f"{fam} {loss}: exact {ref['exact'] / B:.3f} acc {ref['acc'] / B:.4f} acc_thr {ref['acc_thr'] / B:.4f} "
              f"undecided rows {ref['near_rows'] / B:.4f}")
        assert ref["count"] == B
        assert ref["near_rows"] <= 0.02 * B, (fam, ref["near_rows"])
        assert np.isfinite(ref["loss"])
        if fam == "signal":
            assert 0.05 < ref["exact"] / B < 0.95
        if fam == "integers":
            zz = z[:, :62].double()
            sm, ss = zz[:, :50].sort(1, descending=True).values, zz[:, 50:].sort(1, descending=True).values
            tied = (sm[:, 4] == sm[:, 5]) | (ss[:, 1] == ss[:, 2])
            assert float(tied.double().mean()) >= 0.95
        if fam == "spikes" and loss == "softmax":
            lp = R.log_probs(z.double().numpy()[:, :62])
            assert float((lp >= -R.LN2).any(1).mean()) > 0.9
    # the reference itself breaks ties towards the earlier index
    z = torch.zeros(2, 64)
    y = torch.zeros(2, 62)
    y[0, [0, 1, 2, 3, 4, 50, 51]] = 1
    y[1, [45, 46, 47, 48, 49, 60, 61]] = 1
    m = draw_metrics(z.numpy()[:, :62], y.numpy(), loss)
    assert m["exact"] == 0.5 and m["hits_main"] == 2.5 and m["hits_star"] == 1.0
