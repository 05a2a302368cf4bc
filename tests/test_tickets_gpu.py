"""csrc/tickets.hip (ops.tickets.draw_tickets, the models' tickets() / backtest()) against the fp64 numpy
specification euromillioner_amd.tickets, under the rules of tests/_tickets_ref.py:

* keys_out within tol = 16 x the fp32 error of the formula itself, per element;
* tickets == the stable top-k of the kernel's own keys, exactly; == the fp64 picks outside the near set
  (share <= 0.2 %); bit-equal with and without the optional outputs;
* partials integer-equal, per block, to score_tickets_py of the kernel's own tickets;
* T = 0, N = 1 agrees with em_draw_metrics' hit counts on the same logits;
* back-test integers independent of chunking and of an identity sample index.

Measured on an MI355X (all shapes, T = 1 and 0.25): largest key error 3.2e-6 randn3, 2.0e-6 signal, 2.5e-6 integers,
6.1e-5 randn80, 4.6e-6 spikes, 1.6e-5 hot; the tolerance was 7.8 to 16 times the error in every launch; near pairs 5 to
24 of 153,414 per source (cap 0.2 % = 306).  Nothing here depends on timing."""
import numpy as np
import pytest
import torch

import _fused_ref as R
import _tickets_ref as TR
from euromillioner_amd import tickets as TK

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (5, 3), (257, 1), (70, 64), (1301, 16))
TEMPS = (1.0, 0.25, 0.0)
SEED = 7


@pytest.fixture(scope="module")
def draws():
    return R.draw_masks().cuda()


@pytest.fixture(scope="module")
def hot_model():
    from euromillioner_amd.models.mlp import FusedSmallMLP

    return FusedSmallMLP(state_dict=R.make_state("hot"))


def _logits(source, hot_model, draws, B, off, sidx=None):
    """[B, 64] fp32 GPU logits of one source: a _fused_ref family, or the hot model's own logits()."""
    if source == "hot":
        return hot_model.logits(draws, B, offset=off, sidx=None if sidx is None else sidx.cuda()).clone()
    _, Y = R.xy(R.draw_masks(), B, off, sidx=sidx)
    return R.logit_family(source, Y, seed=B + off).cuda()


def _rows_per_block(n):
    p = 1
    while p < n:
        p *= 2
    return 256 // p


def _check_case(lg, draws, B, N, T, off=0, sidx=None, row_base=0, stats=None):
    """Every per-launch check for one (logits, shape, T, indexing)."""
    from euromillioner_amd.ops import tickets as OT

    si = None if sidx is None else sidx.cuda()
    full = OT.draw_tickets(lg, B, N, T, SEED, masks=draws, offset=off, sidx=si, row_base=row_base, want_keys=True)
    lean = OT.draw_tickets(lg, B, N, T, SEED, masks=draws, offset=off, sidx=si, row_base=row_base)
    bare = OT.draw_tickets(lg, B, N, T, SEED, offset=off, sidx=si, row_base=row_base)
    none = OT.draw_tickets(lg, B, N, T, SEED, masks=draws, offset=off, sidx=si, row_base=row_base,
                           want_tickets=False)
    assert set(bare) == {"tickets"} and set(none) == {"partials"}
    assert torch.equal(full["tickets"], lean["tickets"]) and torch.equal(full["tickets"], bare["tickets"])
    assert torch.equal(full["partials"], lean["partials"]) and torch.equal(full["partials"], none["partials"])
    tk = full["tickets"].cpu().numpy().view(np.uint64)
    keys = full["keys"].cpu().numpy()
    part = full["partials"].cpu().numpy()
    assert tk.shape == (B, N) and keys.shape == (B, N, 64)

    idx = sidx[:B].long().numpy() if sidx is not None else np.arange(off, off + B)
    k = TK.ticket_uniform_bits(SEED, [row_base + int(i) for i in idx], N)
    tol, keys64 = TR.key_tol(lg.cpu().numpy(), k, T)
    err = TR.check_keys(keys, keys64, tol)
    TR.check_own_keys(tk, keys)
    st = TR.check_vs_spec(tk, keys64, tol)

    targets = R.draw_masks().numpy().view(np.uint64)[idx + 1]
    rpb = _rows_per_block(N)
    assert part.shape == (OT.ticket_blocks(B, N), 32) and part.shape[0] == (B + rpb - 1) // rpb
    for b in range(part.shape[0]):
        sl = slice(b * rpb, min((b + 1) * rpb, B))
        h, bt = TK.score_tickets_py(tk[sl], targets[sl])
        assert np.array_equal(part[b, :18].astype(np.int64), h.reshape(-1)), (b, part[b], h)
        assert np.array_equal(part[b, 18:].astype(np.int64), bt), (b, part[b], bt)
    hist, best = OT.sum_partials(full["partials"])
    assert hist.sum() == B * N and best.sum() == B
    if stats is not None:
        stats["max_err"] = max(stats.get("max_err", 0.0), err)
        stats["max_tol"] = max(stats.get("max_tol", 0.0), tol)
        stats["min_slack"] = min(stats.get("min_slack", np.inf), tol / err if err > 0 else np.inf)
        stats["near"] = stats.get("near", 0) + st["near"]
        stats["pairs"] = stats.get("pairs", 0) + st["pairs"]
    return tk


@pytest.mark.parametrize("source", R.FAMILIES + ("hot",))
def test_draw_tickets_matches_spec(draws, hot_model, source):
    stats = {}
    for B, N in SHAPES:
        for off in (0, 17):
            lg = _logits(source, hot_model, draws, B, off)
            for T in TEMPS:
                _check_case(lg, draws, B, N, T, off=off, stats=stats)
    print(f"{source}: max key error {stats['max_err']:.3e} (largest tol {stats['max_tol']:.3e}, smallest "
          f"tol / error {stats['min_slack']:.1f}); near pairs {stats['near']} of {stats['pairs']}")
    TR.check_near_share(stats["near"], stats["pairs"])


def test_sample_index_and_row_base(draws, hot_model):
    """A shuffled sample index with repeats (a repeated row gives identical tickets), and row ids past 2^33."""
    B, N = 1301, 16
    sidx = torch.randint(0, 5000, (B,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    sidx[250:262] = sidx[0]
    stats = {}
    for source in ("randn3", "hot"):
        lg = _logits(source, hot_model, draws, B, 0, sidx=sidx)
        for T in (1.0, 0.0):
            tk = _check_case(lg, draws, B, N, T, sidx=sidx, stats=stats)
            if source == "hot":  # the model's logits of a repeated draw are the same row
                assert (tk[250:262] == tk[0]).all()
    lg = _logits("randn3", hot_model, draws, 70, 17)
    a = _check_case(lg, draws, 70, 64, 1.0, off=17, row_base=2 ** 33, stats=stats)
    b = _check_case(lg, draws, 70, 64, 1.0, off=17, stats=stats)
    TR.check_near_share(stats["near"], stats["pairs"])
    assert (a != b).mean() > 0.9  # another row id, another stream


@pytest.mark.parametrize("family", ["integers", "randn3"])
def test_greedy_agrees_with_draw_metrics(draws, family):
    """T = 0, N = 1 is the arg-max pick that em_draw_metrics scores: same hit counts on the same logits."""
    from euromillioner_amd.ops import fused_mlp as FM
    from euromillioner_amd.ops import tickets as OT

    B, off = 1301, 17
    _, Y = R.xy(R.draw_masks(), B, off)
    lg = R.logit_family(family, Y, seed=3).cuda()
    hist, best = OT.sum_partials(OT.draw_tickets(lg, B, 1, 0.0, SEED, masks=draws, offset=off)["partials"])
    dm = FM.draw_metrics(lg, draws, B, offset=off).double().sum(0).cpu().numpy()
    m, s = np.arange(6)[:, None], np.arange(3)[None, :]
    assert (m * hist).sum() == dm[3] and (s * hist).sum() == dm[4] and best[0] == dm[5] and hist.sum() == dm[7]
    assert (m * hist).sum() > 0


def _gemm_state(n_in, seed=4):
    from euromillioner_amd.models.mlp import DrawMLP

    sd = {k: v.clone() for k, v in DrawMLP((n_in, 96, 62), seed=seed).state_dict().items()}
    sd["layers.0.weight"] *= 3.0
    sd["layers.1.weight"] *= 3.0
    sd["layers.0.bias"] = 0.5 * torch.randn(96, generator=torch.Generator().manual_seed(seed))
    sd["layers.1.bias"] = R.make_state("biased")["l2.bias"].clone()
    return sd


def _make(kind):
    if kind.startswith("gemm"):
        from euromillioner_amd.models.gemm_mlp import GemmMLPTrainer

        lags = 2 if kind == "gemm-lags2" else 1
        return GemmMLPTrainer((62 * lags, 96, 62), state_dict=_gemm_state(62 * lags), lags=lags), lags
    from euromillioner_amd.models.mlp import FusedSmallMLP

    return FusedSmallMLP(state_dict=R.make_state("biased"), dtype=kind), 1


@pytest.mark.parametrize("kind", ["bf16", "fp32", "gemm", "gemm-lags2"])
def test_backtest_chunks_and_sample_index(draws, kind):
    """backtest() at B = 1301 from offset 5: identical integers in chunks of 500, in one chunk and through an
    identity sample index, equal to the spec applied to the model's own logits() (near-set rule); with lags = 2
    the target is draw i + 2."""
    m, lags = _make(kind)
    B, off, N, T = 1301, 5, 16, 1.0
    ident = torch.arange(off, off + B, dtype=torch.int32, device="cuda")
    runs = {"chunk=500": m.backtest(draws, B, N, T, SEED, offset=off, chunk=500),
            "default": m.backtest(draws, B, N, T, SEED, offset=off),
            "sidx": m.backtest(draws, B, N, T, SEED, sidx=ident, chunk=500)}
    base = runs["default"]
    for name, r in runs.items():
        assert np.array_equal(r["hist"], base["hist"]) and np.array_equal(r["best"], base["best"]), name
        assert r["rows"] == B and r["tickets"] == B * N and r["hist"].sum() == B * N and r["best"].sum() == B
        assert abs(r["uniform"]["hist"].sum() - B * N) < 1e-6 and abs(r["uniform"]["best"].sum() - B) < 1e-6
    z = m.logits(draws, B, offset=off).clone().cpu().numpy()
    k = TK.ticket_uniform_bits(SEED, np.arange(off, off + B), N)
    tol, keys64 = TR.key_tol(z, k, T)
    targets = R.draw_masks().numpy().view(np.uint64)[np.arange(off, off + B) + lags]
    st = TR.check_counts_vs_spec(base["hist"], base["best"], TK.tickets_from_keys(keys64), targets, keys64, tol)
    print(f"{kind}: {st}")
    if lags > 1:  # the unshifted target gives other integers: the shift is observable
        wrong = TK.score_tickets_py(TK.tickets_from_keys(keys64),
                                    R.draw_masks().numpy().view(np.uint64)[np.arange(off, off + B) + 1])
        assert not np.array_equal(wrong[0], base["hist"])
    if kind == "bf16":
        tk = m.tickets(draws, B, N, T, SEED, offset=off).cpu().numpy().view(np.uint64)
        h, bt = TK.score_tickets_py(tk, targets)
        assert np.array_equal(h, base["hist"]) and np.array_equal(bt, base["best"])


def test_argument_errors(draws):
    from euromillioner_amd.ops import tickets as OT

    lg = torch.zeros(8, 64, device="cuda")
    for kw in ({"n_tickets": 0}, {"n_tickets": 65}, {"temperature": -1.0}, {"temperature": float("nan")}):
        args = {"n_tickets": 4, "temperature": 1.0, **kw}
        with pytest.raises(ValueError):
            OT.draw_tickets(lg, 8, args["n_tickets"], args["temperature"], SEED, masks=draws)
    short = draws[:20]
    with pytest.raises(ValueError):
        OT.draw_tickets(lg, 8, 4, 1.0, SEED, masks=short, offset=12)  # needs offset + B + 1 = 21 draws
    OT.draw_tickets(lg, 8, 4, 1.0, SEED, masks=short, offset=11)
    with pytest.raises(ValueError):
        OT.draw_tickets(lg[:, :32], 8, 4, 1.0, SEED)
