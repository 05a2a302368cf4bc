"""The forest fit reference ``_rf_fit_ref.check_forest`` is itself checked (no GPU): a forest computed by hand,
the numpy engine on the small cases the GPU tests use, and one mutation per way a fitted forest can be wrong --
each must be rejected with the offending tree, node and field named."""
import numpy as np
import pytest

from euromillioner_amd.models import forest as FO
from euromillioner_amd.models.forest_oracle import grow_forest_numpy

from _rf_fit_cases import SMALL_CASES
from _rf_fit_ref import ForestMismatch, check_forest

# ---------------------------------------------------------------------------------------------- by hand
HAND_SEED, HAND_MIN_LEAF = 3, 3
HAND_W = [0, 2, 3, 2, 1, 3, 0, 4, 0, 0, 1, 1]  # poisson_weights(3, 0, 12): rows 0, 6, 8, 9 are out of the bag
#          row:  0        1        2        3        4        5        6        7        8        9        10       11
HAND_X = [(1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1), (1, 0, 1), (1, 1, 1), (1, 1, 1),
          (0, 1, 1), (1, 1, 1)]
HAND_Y = [(1, 1), (0, 0), (1, 0), (0, 1), (1, 1), (0, 0), (1, 1), (1, 0), (1, 1), (1, 1), (0, 1), (1, 0)]


def _hand_problem():
    X = FO.pack_bits(np.array(HAND_X))
    Y = FO.pack_bits(np.array(HAND_Y))[:, 0].copy()
    return X, Y


def _hand_forest():
    """Depth 2, F = k = 3 (every feature is a candidate), min_samples_leaf 3, n = 17 over 8 kept rows.

    root (n 17, S = (9, 4), s2 = 97):
      f0: right = rows 2, 4, 7, 11: nR 9, SR (9, 1), aR 82; nL 8, SL (0, 3), aL 9:   9/8 + 82/9 - 97/17 = 4.530
      f1: right = rows 3, 4, 10, 11: nR 5, SR (2, 4), aR 20; nL 12, SL (7, 0), aL 49: 49/12 + 20/5 - 97/17 = 2.377
      f2: right = rows 5, 7, 10, 11: nR 9, SR (5, 1), aR 26; nL 8, SL (4, 3), aL 25:  25/8 + 26/9 - 97/17 = 0.308
      -> f0.
    node 1 (x0 = 0: rows 1, 3, 5, 10; n 8, S (0, 3), s2 9):
      f0: nR 0, out;  f1: right = rows 3, 10: nR 3, SR (0, 3), aR 9; nL 5, aL 0: 0/5 + 9/3 - 9/8 = 1.875
      f2: right = rows 5, 10: nR 4, SR (0, 1), aR 1; nL 4, SL (0, 2), aL 4: 4/4 + 1/4 - 9/8 = 0.125  -> f1.
    node 2 (x0 = 1: rows 2, 4, 7, 11; n 9, S (9, 1), s2 82):
      f0: nL 0, out;  f1: right = rows 4, 11: nR 2 < 3, out (its gain, 49/7 + 5/2 - 82/9 = 0.389, would have won)
      f2: right = rows 7, 11: nR 5, SR (5, 0), aR 25; nL 4, SL (4, 1), aL 17: 17/4 + 25/5 - 82/9 = 0.139  -> f2.
    leaves: node 3 = rows 1, 5 (n 5, S (0, 0)); 4 = rows 3, 10 (n 3, S (0, 3)); 5 = rows 2, 4 (n 4, S (4, 1));
            6 = rows 7, 11 (n 5, S (5, 0))."""
    feat = np.array([[0, 1, 2, -1, -1, -1, -1]], dtype=np.int16)
    gain = np.array([[9 / 8 + 82 / 9 - 97 / 17, 0 / 5 + 9 / 3 - 9 / 8, 17 / 4 + 25 / 5 - 82 / 9, 0, 0, 0, 0]])
    cover = np.array([[17, 8, 9, 5, 3, 4, 5]], dtype=np.float32)
    value = np.zeros((1, 7, 64), dtype=np.float32)
    value[0, :, :2] = np.array([(9 / 17, 4 / 17), (0, 3 / 8), (1, 1 / 9), (0, 0), (0, 1), (1, 1 / 4), (1, 0)]).astype(np.float32)
    return feat, value, gain, cover


def _hand_check(arrays, trees=range(1)):
    X, Y = _hand_problem()
    return check_forest(X, Y, 3, *arrays, trees, 2, 3, HAND_MIN_LEAF, True, HAND_SEED)


def test_hand_forest_depth2_min_leaf_weights():
    assert FO.poisson_weights(HAND_SEED, 0, 12).tolist() == HAND_W and max(HAND_W) >= 2
    hand = _hand_forest()
    rep = _hand_check(hand)
    assert rep.reached == [1, 2, 4] and rep.max_rows == [8, 4, 2] and rep.max_flat == [0, 1, 3] and rep.splits == 3
    X, Y = _hand_problem()
    eng = grow_forest_numpy(X, Y, 3, [0], 2, 3, HAND_MIN_LEAF, True, HAND_SEED)
    for a, b in zip(hand, eng):
        assert np.array_equal(a, b)
    assert hand[2][0, 0] == pytest.approx(4.5302, abs=1e-4)  # (the docstring's decimals)


# ---------------------------------------------------------------------------------------------- the numpy engine
@pytest.mark.parametrize("case", SMALL_CASES, ids=repr)
def test_accepts_numpy_engine(case):
    X, Y, F, k = case.load()
    arrays = grow_forest_numpy(X, Y, F, list(case.trees), case.depth, k, case.min_leaf, case.bootstrap, case.seed)
    rep = check_forest(X, Y, F, *arrays, case.trees, case.depth, k, case.min_leaf, case.bootstrap, case.seed)
    assert rep.reached[0] == len(case.trees)
    assert rep.nodes == int((arrays[0] > -2).sum())
    assert rep.splits == int((arrays[0] >= 0).sum())


def test_small_cases_cover_what_they_claim():
    """The cases must keep reaching the situations they exist for."""
    by = {c.name: c for c in SMALL_CASES}
    X, Y, F, k = by["minleaf400-boot"].load()
    f, _, _, cov = grow_forest_numpy(X, Y, F, [0], 6, k, 400, True, 11)
    inner = slice(0, (1 << 6) - 1)  # above max_depth
    assert ((f[0, inner] == -1) & (cov[0, inner] < 800)).any(), "no node fails n >= 2 * min_leaf"
    assert (f[0, inner] >= 0).sum() > 1
    c = by["n1-boot"]
    X, Y, F, k = c.load()
    cov = grow_forest_numpy(X, Y, F, list(c.trees), c.depth, k, 1, True, c.seed)[3]
    assert (cov[:, 0] == 0).any() and (cov[:, 0] > 0).any(), "n = 1 with bootstrap: want an empty and a kept root"
    X, Y, F, k = by["y_zero-all"].load()
    assert (grow_forest_numpy(X, Y, F, [0, 1], 3, k, 1, False, 11)[0][:, 0] == -1).all()


# ---------------------------------------------------------------------------------------------- mutations
M_DEPTH, M_K, M_LEAF, M_SEED, M_TREES = 4, 8, 30, 5, range(2, 4)


@pytest.fixture(scope="module")
def base():
    from _rf_fit_cases import draws_data

    X, Y, F = draws_data(700, 1)
    arrays = grow_forest_numpy(X, Y, F, list(M_TREES), M_DEPTH, M_K, M_LEAF, True, M_SEED)
    for a in arrays:
        a.setflags(write=False)
    check_forest(X, Y, F, *arrays, M_TREES, M_DEPTH, M_K, M_LEAF, True, M_SEED)
    return X, Y, F, arrays


def _rejects(base, mutate, tree, node, fld):
    X, Y, F, arrays = base
    feat, value, gain, cover = (a.copy() for a in arrays)
    mutate(feat, value, gain, cover)
    with pytest.raises(ForestMismatch) as e:
        check_forest(X, Y, F, feat, value, gain, cover, M_TREES, M_DEPTH, M_K, M_LEAF, True, M_SEED)
    assert (e.value.tree, e.value.node, e.value.field) == (tree, node, fld), str(e.value)
    assert f"tree {tree} node {node}" in str(e.value)


def _split_node(base, ti=1, level=2):
    feat = base[3][0]
    for node in range((1 << level) - 1, (2 << level) - 1):
        if feat[ti, node] >= 0:
            return node
    raise AssertionError("no split node at that level")


def test_rejects_feat_other_candidate(base):
    node = _split_node(base)
    cs = FO.candidates(M_SEED, M_TREES[1], node, base[2], M_K)
    other = int([c for c in cs if c != base[3][0][1, node]][0])
    _rejects(base, lambda f, v, g, c: f.__setitem__((1, node), other), M_TREES[1], node, "feat")


def test_rejects_feat_non_candidate(base):
    node = _split_node(base)
    cs = set(FO.candidates(M_SEED, M_TREES[1], node, base[2], M_K).tolist())
    other = [f for f in range(base[2]) if f not in cs][0]
    _rejects(base, lambda f, v, g, c: f.__setitem__((1, node), other), M_TREES[1], node, "feat")


def test_rejects_split_made_leaf(base):
    node = _split_node(base)

    def m(f, v, g, c):
        f[1, node], g[1, node] = -1, 0.0
    _rejects(base, m, M_TREES[1], node, "feat")


def _inner_leaf(base, ti=0):
    feat = base[3][0]
    for node in range(1, (1 << M_DEPTH) - 1):
        if feat[ti, node] == -1:
            return node
    raise AssertionError("no leaf above max_depth")


def test_rejects_leaf_made_split(base):
    node = _inner_leaf(base)  # a reached leaf above max_depth: no admissible candidate gains
    _rejects(base, lambda f, v, g, c: f.__setitem__((0, node), 0), M_TREES[0], node, "feat")
    last = (1 << M_DEPTH) - 1 + int(np.nonzero(base[3][0][0, (1 << M_DEPTH) - 1:] == -1)[0][0])  # a max_depth leaf
    _rejects(base, lambda f, v, g, c: f.__setitem__((0, last), 0), M_TREES[0], last, "feat")


def test_rejects_value_one_ulp(base):
    node = _split_node(base)
    j = int(np.nonzero(base[3][1][1, node] > 0)[0][0])

    def m(f, v, g, c):
        v[1, node, j] = np.nextafter(v[1, node, j], np.float32(2))
    _rejects(base, m, M_TREES[1], node, "value")
    _rejects(base, lambda f, v, g, c: v.__setitem__((1, node, 63), 1e-30), M_TREES[1], node, "value")  # a pad output


def test_rejects_cover_off_by_one(base):
    node = _split_node(base)
    _rejects(base, lambda f, v, g, c: c.__setitem__((1, node), c[1, node] + 1), M_TREES[1], node, "cover")


def test_rejects_gain_one_ulp(base):
    node = _split_node(base)
    _rejects(base, lambda f, v, g, c: g.__setitem__((1, node), np.nextafter(g[1, node], np.inf)), M_TREES[1], node, "gain")


def test_rejects_sibling_values_swapped(base):
    node = _split_node(base)
    a, b = 2 * node + 1, 2 * node + 2

    def m(f, v, g, c):
        v[1, [a, b]] = v[1, [b, a]]
    _rejects(base, m, M_TREES[1], a, "value")


def test_rejects_absent_made_leaf(base):
    leaf = _inner_leaf(base)
    _rejects(base, lambda f, v, g, c: f.__setitem__((0, 2 * leaf + 1), -1), M_TREES[0], 2 * leaf + 1, "feat")


def test_rejects_tie_broken_to_higher_index():
    """Columns 7 and 20 are identical and output 0 equals them: the sums, and so the fp64 gains, are the same
    bits, and the definition takes the lower index."""
    rng = np.random.default_rng(3)
    B = rng.integers(0, 2, size=(300, 62))
    B[:, 20] = B[:, 7]
    Yb = np.zeros((300, 62), dtype=np.int64)
    Yb[:, 0] = B[:, 7]
    Yb[:, 1] = rng.integers(0, 2, size=300)
    X, Y = FO.pack_bits(B), FO.pack_bits(Yb)[:, 0].copy()
    feat, value, gain, cover = grow_forest_numpy(X, Y, 62, [0], 2, 62, 1, False, 1)
    assert feat[0, 0] == 7
    check_forest(X, Y, 62, feat, value, gain, cover, [0], 2, 62, 1, False, 1)
    feat[0, 0] = 20  # the same children, the same gain: only the index is wrong
    with pytest.raises(ForestMismatch) as e:
        check_forest(X, Y, 62, feat, value, gain, cover, [0], 2, 62, 1, False, 1)
    assert (e.value.tree, e.value.node, e.value.field) == (0, 0, "feat")


def test_rejects_split_violating_min_leaf():
    """Node 2 of the hand forest: feature 1 has the larger gain but a right child of weight 2 < 3."""
    feat, value, gain, cover = _hand_forest()
    feat[0, 2], gain[0, 2] = 1, 49 / 7 + 5 / 2 - 82 / 9
    cover[0, 5:7] = (7, 2)
    value[0, 5, :2], value[0, 6, :2] = (1, 0), (1, 0.5)
    with pytest.raises(ForestMismatch) as e:
        _hand_check((feat, value, gain, cover))
    assert (e.value.tree, e.value.node, e.value.field) == (0, 2, "feat")


def test_rejects_wrong_global_tree_id(base):
    X, Y, F, arrays = base
    with pytest.raises(ForestMismatch) as e:
        check_forest(X, Y, F, *arrays, range(M_TREES[0] + 1, M_TREES[0] + 3), M_DEPTH, M_K, M_LEAF, True, M_SEED)
    assert (e.value.tree, e.value.node) == (M_TREES[0] + 1, 0) and e.value.field in ("cover", "value")
    feat, value, gain, cover = _hand_forest()
    with pytest.raises(ForestMismatch) as e:
        _hand_check((feat, value, gain, cover), trees=range(1, 2))
    assert (e.value.tree, e.value.node) == (1, 0)


def test_exact_guard_rejects_a_worse_split():
    """The integer cross-check on its own: a candidate whose exact gain is far below another's is refused."""
    from _rf_fit_ref import _exact_guard

    i64 = lambda *a: np.array(a, dtype=np.int64)  # noqa: E731
    # the hand forest's root: slots f0, f1, f2
    args = (i64(9, 49, 25), i64(82, 20, 26), i64(8, 12, 8), i64(9, 5, 9), 97, 17, np.array([True, True, True]))
    _exact_guard(0, 0, 0, *args)
    with pytest.raises(ForestMismatch):
        _exact_guard(0, 0, 1, *args)
    # an inadmissible better candidate is not held against the choice
    _exact_guard(0, 0, 1, *args[:-1], np.array([False, True, True]))
