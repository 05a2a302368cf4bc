"""The ticket specification euromillioner_amd.tickets (pure numpy), the comparison rules of tests/_tickets_ref.py
checked on deliberately wrong implementations, and the `predict --tickets` / `backtest` command lines on the CPU.

Figures measured when this file was written (B = 1301 rows x 16 tickets per logit source unless stated):
distribution max |z| 1.78 (star inclusion) / 2.05 (main top-1) at 4096 x 16; near share at most 0.03 %."""
import itertools
import json
import math

import numpy as np
import pytest
import torch

import _fused_ref as R
import _tickets_ref as TR
from euromillioner_amd import tickets as TK


# ------------------------------------------------------------------------------------------------ RNG
def test_pins():
    assert TK.ticket_uniform_bits(7, [0], 1)[0, 0, :4].tolist() == [5882177, 5110799, 1080908, 3567437]
    assert TK.ticket_uniform_bits(7, [3], 2)[0, 1, 58:62].tolist() == [7404674, 5040922, 4384141, 4418685]
    assert TK.ticket_uniform_bits(123456789, [2 ** 33 + 5], 64)[0, 63, :2].tolist() == [4225019, 7549724]


def test_bits_range_and_exact_uniforms():
    k = TK.ticket_uniform_bits(7, np.arange(200), 16)
    assert k.shape == (200, 16, 62) and k.dtype == np.uint32
    assert k.min() >= 0 and k.max() < 2 ** 23 and k.max() > 2 ** 23 - 2 ** 12 and k.min() < 2 ** 12
    u64, u32 = TK.uniforms(k, np.float64), TK.uniforms(k, np.float32)
    assert u32.dtype == np.float32 and np.array_equal(u32.astype(np.float64), u64)  # exact in fp32
    assert u64.min() > 0 and u64.max() < 1
    ends = TK.uniforms(np.array([0, 2 ** 23 - 1], dtype=np.uint32), np.float32)
    assert 0 < ends[0] and ends[1] < 1  # never 0 or 1, also after rounding to fp32
    # a ticket's stream depends on t and on the row id, not on how many tickets are asked for
    assert np.array_equal(TK.ticket_uniform_bits(7, [5], 3)[0], k[5, :3])
    assert len({k[i, t].tobytes() for i in range(20) for t in range(16)}) == 320


# ------------------------------------------------------------------------------------------------ distribution
def test_plackett_luce_distribution():
    """4096 rows of identical scores, 16 tickets, seed 7, T = 1: star inclusion frequencies against the closed
    form p_i + sum_{j != i} p_j p_i / (1 - p_j), main top-1 frequencies against softmax, within 4.5 standard
    errors (measured: max |z| 1.78 and 2.05)."""
    B, n = 4096, 16
    sc = np.concatenate([np.linspace(-1, 1, 50), np.linspace(-1.5, 1.5, 12)])
    tks, keys = TK.sample_tickets_py(np.tile(sc, (B, 1)), np.arange(B), n, 1.0, 7)
    cnt = B * n
    ps = np.exp(sc[50:]) / np.exp(sc[50:]).sum()
    incl = np.array([ps[i] + sum(ps[j] * ps[i] / (1 - ps[j]) for j in range(12) if j != i) for i in range(12)])
    assert abs(incl.sum() - 2) < 1e-12
    got = np.array([((tks >> np.uint64(50 + i)) & np.uint64(1)).sum() for i in range(12)]) / cnt
    z_star = (got - incl) / np.sqrt(incl * (1 - incl) / cnt)
    pm = np.exp(sc[:50]) / np.exp(sc[:50]).sum()
    top1 = np.bincount(keys[..., :50].argmax(-1).reshape(-1), minlength=50) / cnt
    z_main = (top1 - pm) / np.sqrt(pm * (1 - pm) / cnt)
    print(f"max |z|: star inclusion {np.abs(z_star).max():.2f}, main top-1 {np.abs(z_main).max():.2f}")
    assert np.abs(z_star).max() < 4.5 and np.abs(z_main).max() < 4.5


# ------------------------------------------------------------------------------------------------ near ties
def _sources(B):
    masks = R.draw_masks()
    X, Y = R.xy(masks, B, 3)
    out = {f: R.logit_family(f, Y, seed=1).numpy() for f in R.FAMILIES}
    out["hot"] = R.ref_forward(R.make_state("hot"), X, bf16=True).float().numpy()  # hot-scale scores
    return out


@pytest.fixture(scope="module")
def sources():
    return _sources(1301)


@pytest.fixture(scope="module")
def bits():
    return TK.ticket_uniform_bits(7, np.arange(3, 3 + 1301), 16)


@pytest.mark.parametrize("T", [1.0, 0.25])
def test_near_tie_cap(sources, bits, T):
    """tol = 16 x the fp32 error of the formula; at most 0.2 % of (row, ticket) pairs may lie within 2 tol of
    another pick (measured: at most 0.03 %, tol at most 5e-4 at |key| ~ 730)."""
    for name, z in sources.items():
        tol, k64 = TR.key_tol(z, bits, T)
        near = TR.near_set(k64, tol)
        print(f"T={T} {name}: tol {tol:.2e} max |key| {np.abs(k64).max():.0f} near {near.mean():.4%}")
        TR.check_near_share(int(near.sum()), near.size)
        # the fp32 evaluation of the formula passes the rules the kernel is held to
        k32 = TK.keys_from_bits(z.astype(np.float32), bits, T, np.float32)
        TR.check_keys(k32, k64, tol)
        tk32 = TK.tickets_from_keys(k32.astype(np.float64))
        TR.check_own_keys(tk32, k32)
        TR.check_vs_spec(tk32, k64, tol)


# ------------------------------------------------------------------------------------------------ greedy
def test_greedy_is_top_pick(sources):
    from euromillioner_amd.train import _top_pick

    for name in ("integers", "randn3", "hot"):  # integers: ties across the top-5 / top-2 boundary
        z = sources[name][:200]
        tks, keys = TK.sample_tickets_py(z, np.arange(200), 3, 0.0, 7)
        assert np.array_equal(keys, np.broadcast_to(z[:, None, :62].astype(np.float64), keys.shape))
        for r in range(200):
            main, stars = _top_pick(z[r].astype(np.float64))
            for t in range(3):
                assert TK.ticket_numbers(tks[r, t]) == (main, stars), (name, r, t)


# ------------------------------------------------------------------------------------------------ tiers
def test_tier_table_and_uniform_play():
    assert TK.TIER_RANK.shape == (6, 3) and len(TK.TIER_NAMES) == 14
    ranks = TK.TIER_RANK.reshape(-1).tolist()
    assert sorted(r for r in ranks if r != 14) == list(range(1, 14)) and ranks.count(14) == 5  # bijection + none
    for m, s in itertools.product(range(6), range(3)):
        r = TK.TIER_RANK[m, s]
        assert TK.TIER_NAMES[r - 1] == (f"{m}+{s}" if r < 14 else "none")
    assert [(m, s) for m in range(6) for s in range(3) if TK.TIER_RANK[m, s] == 14] == \
        [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
    u = TK.uniform_expectation(1)
    assert abs(u["hist"].sum() - 1) < 1e-12 and abs(u["rank"].sum() - 1) < 1e-12
    assert abs(1 / u["hist"][5, 2] - 139_838_160) < 1e-3 and u["rank"][0] == u["hist"][5, 2]
    assert np.allclose(u["best"], u["rank"], rtol=0, atol=1e-15)  # one ticket: its own rank
    for n in (2, 16, 64):
        un = TK.uniform_expectation(n)
        assert abs(un["best"].sum() - 1) < 1e-12 and (un["best"] >= 0).all()
        assert math.isclose(un["best"][13], u["rank"][13] ** n, rel_tol=1e-12)  # every ticket without a prize
        assert math.isclose(un["best"][0], 1 - (1 - u["rank"][0]) ** n, rel_tol=1e-6)
    with pytest.raises(ValueError):
        TK.uniform_expectation(0)


def test_score_tickets_brute_force():
    g = np.random.default_rng(3)

    def rand_mask():
        return sum(1 << int(i) for i in g.choice(50, 5, replace=False)) | \
            sum(1 << (50 + int(i)) for i in g.choice(12, 2, replace=False))

    B, n = 300, 5
    tks = np.array([[rand_mask() for _ in range(n)] for _ in range(B)], dtype=np.uint64)
    tg = np.array([rand_mask() for _ in range(B)], dtype=np.uint64)
    tks[:40, 0] = tg[:40]  # some jackpots and near misses
    tks[40:80, 1] = tg[40:80] ^ np.uint64(1 << 50 | 1 << 51 | 1 << 52 | 1 << 53)
    hist, best = np.zeros((6, 3), dtype=np.int64), np.zeros(14, dtype=np.int64)
    for r in range(B):
        tm, ts = map(set, TK.ticket_numbers(tg[r]))
        rk = []
        for t in range(n):
            m, s = map(set, TK.ticket_numbers(tks[r, t]))
            hist[len(m & tm), len(s & ts)] += 1
            rk.append(int(TK.TIER_RANK[len(m & tm), len(s & ts)]))
        best[min(rk) - 1] += 1
    h, b = TK.score_tickets_py(tks, tg)
    assert np.array_equal(h, hist) and np.array_equal(b, best)
    assert h.sum() == B * n and b.sum() == B and b[0] >= 40
    assert np.array_equal(TK.tier_counts(h)[:13], [h[m, s] for r in range(1, 14)
                                                    for m in range(6) for s in range(3) if TK.TIER_RANK[m, s] == r])


# ------------------------------------------------------------------------------------------------ discrimination
@pytest.mark.parametrize("mutation", ["swap_hi_lo", "ignore_t"])
def test_rules_reject_wrong_keys(sources, bits, mutation):
    z = sources["randn3"]
    tol, k64 = TR.key_tol(z, bits, 1.0)
    bad = TR.mutated_keys(z, bits, 1.0, mutation)
    with pytest.raises(AssertionError):
        TR.check_keys(bad, k64, tol)
    with pytest.raises(AssertionError):
        TR.check_vs_spec(TK.tickets_from_keys(bad.astype(np.float64)), k64, tol)


def test_rules_reject_unstable_topk(sources, bits):
    z = sources["integers"]
    tol, k64 = TR.key_tol(z, bits, 0.0)
    assert tol == 0.0
    good = TK.tickets_from_keys(k64)
    TR.check_own_keys(good, k64)
    TR.check_vs_spec(good, k64, tol)
    bad = TR.unstable_tickets(k64)
    assert (bad != good).mean() > 0.5
    with pytest.raises(AssertionError):
        TR.check_own_keys(bad, k64)
    with pytest.raises(AssertionError):
        TR.check_vs_spec(bad, k64, tol)
    h, b = TK.score_tickets_py(bad, R.draw_masks().numpy().view(np.uint64)[4:4 + 1301])
    with pytest.raises(AssertionError):
        TR.check_counts_vs_spec(h, b, good, R.draw_masks().numpy().view(np.uint64)[4:4 + 1301], k64, tol)


# ------------------------------------------------------------------------------------------------ config / CLI
def test_ticket_config_validation():
    from euromillioner_amd import config as C

    assert C.build_config(None, {}, environ={}).tickets.n == 0
    cfg = C.build_config(None, {"tickets.n": "64", "tickets.temperature": "0", "tickets.seed": "9"}, environ={})
    assert (cfg.tickets.n, cfg.tickets.temperature, cfg.tickets.seed) == (64, 0.0, 9)
    for bad in ({"tickets.n": 65}, {"tickets.n": -1}, {"tickets.temperature": -0.5},
                {"tickets.temperature": float("nan")}, {"tickets.temperature": float("inf")}):
        with pytest.raises(ValueError):
            C.build_config(None, bad, environ={})


DATA = ["--n-draws", "900", "--planted", "0.8", "--device", "cpu"]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from euromillioner_amd.cli import main

    path = str(tmp_path_factory.mktemp("tickets") / "mlp.zip")
    assert main(["train", "--model", "mlp", "--steps", "30", "--batch", "128", "--eval-every", "0", "--ckpt", path,
                 "--log-level", "ERROR"] + DATA) == 0
    return path


def _run(capsys, args):
    from euromillioner_amd.cli import main

    capsys.readouterr()
    rc = main(args + ["--log-level", "ERROR"])
    return rc, capsys.readouterr().out.splitlines()


def test_cli_predict_tickets(ckpt, capsys):
    rc, plain = _run(capsys, ["predict", "--ckpt", ckpt] + DATA)
    assert rc == 0 and len(plain) == 2  # the pick and the JSON line, as before this feature
    res0 = json.loads(plain[1])
    assert list(res0) == ["model", "checkpoint", "after_draw", "next_draw_date", "main", "stars", "p_main", "p_stars"]
    rc, out = _run(capsys, ["predict", "--ckpt", ckpt, "--tickets", "5"] + DATA)
    assert rc == 0 and len(out) == 7 and out[0] == plain[0]  # 6 ticket lines + JSON
    res = json.loads(out[6])
    assert {k: res[k] for k in res0} == res0
    assert len(res["tickets"]) == 5
    for t, line in zip(res["tickets"], out[1:6]):
        assert len(t["main"]) == 5 and len(t["stars"]) == 2 and t["main"] == sorted(set(t["main"]))
        assert line == " ".join(f"{v:02d}" for v in t["main"]) + "  *  " + " ".join(f"{v:02d}" for v in t["stars"])
    assert len({json.dumps(t) for t in res["tickets"]}) > 1  # sampled, not five copies of the mode
    _, again = _run(capsys, ["predict", "--ckpt", ckpt, "--tickets", "5"] + DATA)
    assert again == out
    _, other = _run(capsys, ["predict", "--ckpt", ckpt, "--tickets", "5", "--ticket-seed", "1"] + DATA)
    assert other[0] == out[0] and other[1:6] != out[1:6]
    _, greedy = _run(capsys, ["predict", "--ckpt", ckpt, "--tickets", "3", "--temperature", "0"] + DATA)
    assert greedy[1:4] == [plain[0]] * 3
    assert _run(capsys, ["predict", "--ckpt", ckpt, "--tickets", "65"] + DATA)[0] == 2
    assert _run(capsys, ["predict", "--ckpt", ckpt, "--tickets", "2", "--temperature", "-1"] + DATA)[0] == 2


def test_cli_backtest_cpu(ckpt, capsys):
    rc, out = _run(capsys, ["backtest", "--ckpt", ckpt, "--tickets", "4"] + DATA)
    assert rc == 0 and len(out) == 15  # header, 13 tiers, JSON
    res = json.loads(out[-1])
    rows = res["rows"]
    assert rows == 899 - int(899 * 0.7) and res["engine"] == "numpy" and res["tickets"] == rows * 4
    assert np.sum(res["hist"]) == rows * 4 and np.sum(res["best"]) == rows and np.sum(res["tiers"]) == rows * 4
    assert abs(np.sum(res["uniform"]["hist"]) - rows * 4) < 1e-6 and abs(np.sum(res["uniform"]["best"]) - rows) < 1e-6
    for k, line in enumerate(out[1:14]):
        f = line.replace("|", " ").split()
        assert f[:2] == [str(k + 1), TK.TIER_NAMES[k]] and int(f[2]) == res["tiers"][k] and int(f[4]) == res["best"][k]
    _, again = _run(capsys, ["backtest", "--ckpt", ckpt, "--tickets", "4"] + DATA)
    assert again == out
    _, other = _run(capsys, ["backtest", "--ckpt", ckpt, "--tickets", "4", "--ticket-seed", "1"] + DATA)
    assert json.loads(other[-1])["hist"] != res["hist"]
    assert _run(capsys, ["backtest", "--ckpt", ckpt, "--tickets", "65"] + DATA)[0] == 2
    assert _run(capsys, ["backtest", "--ckpt", ckpt] + DATA)[0] == 3  # no tickets asked for


def test_cli_backtest_matches_spec_by_hand(ckpt, capsys):
    """The numbers of `backtest --device cpu` are the specification applied to DrawMLP's logits."""
    from euromillioner_amd import config as C
    from euromillioner_amd.data.draws import lag_features, mask_bits, positional_split
    from euromillioner_amd.models.mlp import DrawMLP
    from euromillioner_amd.pipeline import load_draws
    from euromillioner_amd.train import load_mlp_checkpoint

    _, out = _run(capsys, ["backtest", "--ckpt", ckpt, "--tickets", "4", "--temperature", "0.5"] + DATA)
    res = json.loads(out[-1])
    ds = load_draws(C.build_config(None, {"data.n_draws": 900, "data.planted": 0.8}, environ={}))
    ck = load_mlp_checkpoint(ckpt)
    net = DrawMLP(ck["sizes"], use_hip=False)
    net.load_state_dict(ck["state_dict"])
    X, _ = lag_features(ds.numbers, 1)
    margin = positional_split(len(X), 70.0)
    with torch.no_grad():
        z = net(torch.from_numpy(X[margin:])).numpy()
    tks, _ = TK.sample_tickets_py(z, np.arange(margin, len(X)), 4, 0.5, 0)
    h, b = TK.score_tickets_py(tks, mask_bits(ds.numbers)[1:][margin:])
    assert res["hist"] == h.tolist() and res["best"] == b.tolist()
