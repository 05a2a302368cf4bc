"""The GBDT fit on the device (``em_gbdt_fit`` and the ``em_gbdt_dp_*`` path) against the fp64 regrow of
tests/_gbdt_fit_ref.py: every tree of every fit is regrown from the definition, from the model's own earlier
trees, and ``status``, ``feat``, ``sbin``, ``leaf``, ``gain`` and ``cover`` are compared inside budgets computed
from the reference alone (proved on the CPU by tests/test_gbdt_fit_ref_cpu.py, which also runs every case below
on the numpy engine's trees, so the ambiguity cap is known to be a property of the inputs).

Every case: ``backend_used == "hip"``, no violations, ``ambiguous <= max(1, decisions // 100)``, and a
``FIT-RATIO`` line with the worst |dev - ref| / budget of leaf, gain and cover (``pytest -s``).  Where the numpy
engine fits the case cheaply its ``status``, ``feat`` and ``sbin`` must equal the device's.  The cases and the
row counts that select the split kernel's forms: tests/_gbdt_fit_cases.py."""
import functools
import os
import re

import numpy as np
import pytest

import _gbdt_fit_cases as K
import _gbdt_fit_ref as FR
from euromillioner_amd.models import gbdt as G

pytestmark = pytest.mark.gpu

DRIVERS = ("default", "separate")
TREE_ARRAYS = ("status", "feat", "sbin", "leaf", "gain", "cover")
_fits: dict = {}


def _new(objective, driver="default", backend="hip", **kw):
    g = G.GBDT(objective=objective, backend=backend, **kw)
    g.separate_launches = driver == "separate"
    return g


def _hip(case, driver="default", **over):
    """The HIP fit of a case of K.CASES (fitted once per configuration)."""
    key = (case, driver, tuple(sorted(over.items())))
    if key not in _fits:
        dn, objective, kw = K.CASES[case]
        X, Y, _ = K.data(dn)
        m = _new(objective, driver, **dict(kw, **over)).fit(X, Y)
        assert m.backend_used == "hip"
        _fits[key] = m
    return _fits[key]


@functools.lru_cache(maxsize=None)
def _oracle(case, **over):
    dn, objective, kw = K.CASES[case]
    X, Y, _ = K.data(dn)
    return _new(objective, backend="numpy", **dict(kw, **dict(over))).fit(X, Y)


def _check(m, case, label, rank=0, oracle=True, **over):
    """The reference on a fitted model; returns its Result."""
    dn = K.CASES[case][0]
    X, Y, ties = K.data(dn)
    res = FR.check_fit(m, X, Y, rank=rank, ties=ties)
    print("\n" + res.line(label))
    assert res.violations == [], res.violations[:10]
    assert res.ambiguous <= K.cap(res), (res.ambiguous, res.decisions)
    assert np.isfinite(m.trees.leaf).all()
    if oracle:
        # (two correct engines may part at an ambiguous decision, and from there on: the trees before the first
        # one are compared, which is all of them wherever the reference followed the engine nowhere)
        followed = [r.k for r in res.nodes if r.followed]
        upto = m.trees.n_trees if not res.ambiguous else (min(followed) if len(followed) == res.ambiguous else 0)
        o = _oracle(case, **over)
        for k in ("status", "feat", "sbin"):
            assert np.array_equal(getattr(m.trees, k)[:upto], getattr(o.trees, k)[:upto]), k
    return res


def test_constants_the_shapes_were_derived_from():
    """The row counts, bin counts and depths of the cases below reach the split kernel's forms only while these
    hold; the chunk counts written in tests/_gbdt_fit_cases.py follow from the first."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "gbdt.hip")).read()
    assert re.search(r"#define HIST_MIN_CHUNK (\d+)", src).group(1) == "256"
    assert re.search(r"constexpr int SPLIT_FOLD_MAX_CHUNKS = (\d+)", src).group(1) == "32"
    assert re.search(r"constexpr int SPLIT_ONESHOT_LDS = (\d+) \* (\d+);", src).groups() == ("48", "1024")
    assert re.search(r"constexpr int SPLIT_DIRECT_MAX_BINS = (\d+);", src).group(1) == "32"
    assert re.search(r"constexpr int SPLIT_FINAL_MAX_DEPTH = (\d+);", src).group(1) == "8"
    assert K.HIST_MIN_CHUNK == 256
    for n, (T, chunks) in K.ROWS.items():
        assert K.chunks_of(n, T) == chunks, n
    cells = 124  # 62 one-hot features
    assert 24 * cells * 16 <= 48 * 1024 < 25 * cells * 16  # 2 to 24 chunks staged at once, 25 in the chunk loop
    assert K.ROWS[6400][1] <= 32 < K.ROWS[8448][1]


# ----------------------------------------------------------------------------- 1. drivers x objectives
CASES_1 = [("std-logistic", d) for d in DRIVERS] + [("std-squarederror", d) for d in DRIVERS] + \
    [("std-softprob", "default")]


@pytest.mark.parametrize("case,driver", CASES_1, ids=[f"{c}-{d}" for c, d in CASES_1])
def test_drivers_and_objectives(case, driver):
    m = _hip(case, driver)
    assert (m.trees.status == 1).sum() > m.trees.n_trees
    _check(m, case, f"1 {case} {driver}")


# ----------------------------------------------------------------------------- 2. parameters
@pytest.mark.parametrize("case,driver", [("par-zero", "default"), ("par-zero", "separate"), ("par-heavy", "default"),
                                         ("par-ref", "default")])
def test_parameters(case, driver):
    m = _hip(case, driver)
    res = _check(m, case, f"2 {case} {driver}")
    if case == "par-zero":  # every node inside the corner bound's precondition
        assert res.max_abs_margin <= 8.0 and res.min_open_h > 0
        assert (m.trees.status == 1).sum() > 3 * m.trees.n_trees  # grown well past the roots


@pytest.mark.parametrize("driver", ["default", "separate"])
def test_partial_pruning_gamma(driver):
    """gamma = the median split gain of the gamma = 0 fit: some splits go, some stay, and somewhere a split
    stays whose child lost its own split (a pruned-away grandchild level)."""
    base = _hip("std-logistic")
    gamma = K.partial_gamma(base.trees.gain[base.trees.status == 1])
    m = _hip("std-logistic", driver, gamma=gamma)
    res = _check(m, "std-logistic", f"2 partial gamma {gamma:.6g} {driver}", gamma=gamma)
    st = m.trees.status
    pruned = [r for r in res.nodes if r.split and st[r.k, r.node] == 2]  # the reference split them; now leaves
    assert pruned and (st == 1).sum() > 0
    assert (st == 1).sum() < (base.trees.status == 1).sum()
    assert any(r.node > 0 and st[r.k, (r.node - 1) // 2] == 1 for r in pruned)


# ----------------------------------------------------------------------------- 3. depths
@pytest.mark.parametrize("depth", [1, 6, 8, 9])
def test_depths(depth):
    """Depth 9 = SPLIT_FINAL_MAX_DEPTH + 1 is the smallest past the fused round."""
    m = _hip(f"depth-{depth}")
    assert m.trees.status.shape[1] == 2 ** (depth + 1) - 1
    _check(m, f"depth-{depth}", f"3 depth {depth}")


# ----------------------------------------------------------------------------- 4. row counts
@pytest.mark.parametrize("n", sorted(K.ROWS))
def test_row_counts(n):
    """1 chunk (no fold), 2 (staged at once), 25 (per-cell chunk loop), 33 (gbdt_chunk_reduce)."""
    m = _hip(f"rows-{n}")
    assert m.n_tasks == K.ROWS[n][0]
    _check(m, f"rows-{n}", f"4 rows {n} chunks {K.ROWS[n][1]}")


# ----------------------------------------------------------------------------- 5. feature forms
@pytest.mark.parametrize("case", ["mixed", "cont", "int8"])
def test_feature_forms(case):
    """5a, the reference feature set (one-hot columns and calendar features of 12 to 31 bins on these rows, all
    within SPLIT_DIRECT_MAX_BINS: the direct candidate form over four chunks); 5b, 256-bin features whose scan
    area does not fit beside the partials (the sequential scan); 5c, 8-bin features on two chunks.  The two-pass
    scan runs in the one-chunk row counts and in the 6 x 256-bin multi-class problem."""
    X = K.data(K.CASES[case][0])[0]
    m = _hip(case)
    nb = [len(c) + 1 for c in m.cuts]
    if case == "mixed":  # 62 number columns (a star not drawn yet: one bin), day of week, month, day, year
        assert X.shape == (900, 66) and sum(b == 2 for b in nb) >= 62 and nb[62:] == [2, 12, 31, 13]
    if case == "cont":
        assert min(nb) == 256
    if case == "int8":
        assert X.shape[0] == 257 and max(nb) == 8  # the direct candidate form, two chunks
    _check(m, case, f"5 {case}")


def test_constant_and_duplicated_columns():
    """A constant column first (the node totals are summed from feature 0's cells) and last, a two-valued
    column, and a copy of a one-hot column: an exact tie, which the lower index must win."""
    X, _, ties = K.data("edge")
    m = _hip("edge")
    assert [len(m.cuts[f]) for f in K.EDGE_CONST] == [0, 0] and len(m.cuts[63]) == 1
    _check(m, "edge", "5 edge")
    split_feats = m.trees.feat[m.trees.status == 1]
    assert not np.isin(split_feats, K.EDGE_CONST).any()
    (lo, hi), = ties
    assert (split_feats == lo).any() and not (split_feats == hi).any()


# ----------------------------------------------------------------------------- 6. fixed-point histograms
@pytest.mark.parametrize("case", [c for c in K.CASES if c.startswith("quant-")])
def test_fixed_point_histograms(case):
    m = _hip(case)
    assert m.quant_bits_used > 40
    _check(m, case, f"6 {case}")


# ----------------------------------------------------------------------------- 7. subsampling
CASES_7 = [("sub-0.5-logistic", d) for d in DRIVERS] + [("sub-0.8-logistic", d) for d in DRIVERS] + \
    [("sub-0.5-squarederror", d) for d in DRIVERS] + \
    [(c, "default") for c in ("sub-0.8-quant", "sub-0.5-quant", "sub-0.5-softprob", "sub-0.8-softprob")]


@pytest.mark.parametrize("case,driver", CASES_7, ids=[f"{c}-{d}" for c, d in CASES_7])
def test_subsample(case, driver):
    """The keep mask of hash3(seed, round * 131071 + task, row); the numpy engine draws the same one."""
    m = _hip(case, driver)
    _check(m, case, f"7 {case} {driver}")


@pytest.mark.parametrize("case", ["sub-0.8-rounds7", "sub-0.5-rounds7"])
def test_subsample_chunked_calls(case, monkeypatch):
    """rounds_per_call = 3 over 7 rounds: the mask takes the absolute round, not the chunk's."""
    from euromillioner_amd.models import gbdt_hip

    whole = _hip(case)
    dn, objective, kw = K.CASES[case]
    X, Y, _ = K.data(dn)
    monkeypatch.setattr(gbdt_hip, "fit", functools.partial(gbdt_hip.fit, rounds_per_call=3))
    m = _new(objective, **kw).fit(X, Y)
    assert m.backend_used == "hip"
    for k in TREE_ARRAYS:
        assert np.array_equal(getattr(m.trees, k), getattr(whole.trees, k)), k
    _check(whole, case, f"7 {case} one call")
    _check(m, case, f"7 {case} rounds_per_call 3")


def test_all_rows_dropped():
    """subsample so small that no element is kept, at lambda = 0: H + lambda = 0 at the root, whose leaf is 0
    (XGBoost's CalcWeight), not 0 / 0."""
    m = _hip("dropped-all")
    assert (m.trees.status[:, 0] == 2).all() and (m.trees.leaf == 0).all() and (m.trees.cover == 0).all()
    _check(m, "dropped-all", "7 dropped-all")


# ----------------------------------------------------------------------------- 8. one-rank process group
def test_one_rank_process_group():
    """The data-parallel path (per-level histogram, all-reduce, split) on a one-rank group, without and with
    subsampling: the same checks, ``gain`` and ``cover`` included."""
    import socket

    import torch
    import torch.distributed as dist

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    fits = {}
    try:
        for case in ("std-logistic", "sub-0.5-logistic", "sub-0.8-logistic"):
            dn, objective, kw = K.CASES[case]
            X, Y, _ = K.data(dn)
            fits[case] = _new(objective, **kw).fit(X, Y, group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
    for case, m in fits.items():
        assert m.backend_used == "hip" and m.quant_bits_used == 0
        _check(m, case, f"8 one-rank group {case}", rank=0)


# ----------------------------------------------------------------------------- 9. 62 tasks
def test_62_tasks():
    m = _hip("t62")
    assert m.n_tasks == 62 and m.trees.n_trees == 186
    _check(m, "t62", "9 T = 62")


# ----------------------------------------------------------------------------- 10. launch flags
def test_unknown_launch_flag_is_rejected(monkeypatch):
    """``em_gbdt_fit`` knows one launch flag (1, the separate launches): a call with bit 2 set fails in the
    argument check, before any launch, and ``fit`` raises instead of running some other driver."""
    from euromillioner_amd.models import gbdt_hip

    call = gbdt_hip.N.call

    def with_flag_2(name, *args):
        if name == "em_gbdt_fit":
            args = args[:-2] + (args[-2] | 2,) + args[-1:]
        return call(name, *args)

    dn, objective, kw = K.CASES["std-logistic"]
    X, Y, _ = K.data(dn)
    monkeypatch.setattr(gbdt_hip.N, "call", with_flag_2)
    with pytest.raises(ValueError):
        _new(objective, **kw).fit(X, Y)
