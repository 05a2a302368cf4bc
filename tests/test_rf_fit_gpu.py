"""The device forest driver (``em_rf_fit`` in ``csrc/forest.hip``) on the paths the real workload runs: nodes
split over several blocks (fused record path, mask-form records, index form), the root listing over several
blocks, 256- and 64-thread launches, work lists past one batch and past the LDS block counts, depths to 14,
``min_samples_leaf > 1``, tree-id offsets, feature widths around the record form's limit, tiny and degenerate
sets.  Every fitted tree is checked node by node from the definition (``_rf_fit_ref.check_forest``), and every
case then proves from the reference's report that the path it is named after was taken."""
import numpy as np
import pytest

from euromillioner_amd.models.forest import RandomForest, n_candidates

from _rf_fit_cases import SMALL_CASES, Case, mask_form_data
from _rf_fit_ref import check_forest

gpu = pytest.mark.gpu

# The driver's thresholds, mirrored from csrc/forest.hip.  A retuning there must break a path assertion here.
RF_CHUNK0 = 32768      # RF_CHUNK0: rows per block of a root node (rf_chunk(0))
RF_CHUNK1 = 8192       # RF_CHUNK1: rows per block at level 1
RF_CHUNK = 8192        # RF_CHUNK: rows per block from level 2 on
RF_BEGIN_LDS = 16384   # RF_BEGIN_LDS: work-list items whose block counts rf_level_begin keeps in LDS
RF_SHAPE_NT_ROWS = 2048     # rf_level_threads: (kept >> level) >= 2048 ? 256 : 64
RF_SHAPE_BLOCK_ROWS = 4096  # rf_list_blocks: root listing blocks per tree = N / 4096 (1 .. 64)
RF_BEGIN_BATCH = 8 * 1024   # rf_level_begin: items per batch (PB = 8 per thread x 1024 threads)


def chunk(level):
    return RF_CHUNK0 if level == 0 else RF_CHUNK1 if level == 1 else RF_CHUNK


def blocks(rows, level):
    return max(1, -(-rows // chunk(level)))


def threads(n, bootstrap, level):
    kept = n * 632 // 1000 if bootstrap else n  # em_rf_fit: expected rows per tree
    return 256 if (kept >> level) >= RF_SHAPE_NT_ROWS else 64


def listing_blocks(n):
    return min(64, max(1, n // RF_SHAPE_BLOCK_ROWS))


def row_bytes(X, F):
    from euromillioner_amd.ops import _native as N

    return N.query("em_rf_row_bytes", X.shape[1], F, len(X))


def max_outputs(Y):
    return int(np.unpackbits(np.ascontiguousarray(Y).view(np.uint8)).reshape(len(Y), 64).sum(1).max())


def fit_and_check(case: Case, compare_numpy: bool = False):
    X, Y, F, k = case.load()
    rf = RandomForest(n_trees=len(case.trees), max_depth=case.depth, min_samples_leaf=case.min_leaf,
                      feature_subset=case.subset, bootstrap=case.bootstrap, seed=case.seed, device="cuda")
    rf.fit(X.copy(), Y.copy(), F, trees=case.trees)  # (the shared arrays are read-only)
    assert rf.backend_used == "hip" and rf.k == k
    rep = check_forest(X, Y, F, rf.feat, rf.value, rf.gain, rf.cover, case.trees, case.depth, k, case.min_leaf,
                       case.bootstrap, case.seed)
    if compare_numpy:
        cpu = RandomForest(n_trees=len(case.trees), max_depth=case.depth, min_samples_leaf=case.min_leaf,
                           feature_subset=case.subset, bootstrap=case.bootstrap, seed=case.seed, device="cpu")
        cpu.fit(X, Y, F, trees=case.trees)
        assert np.array_equal(rf.feat, cpu.feat)
        live = rf.feat > -2
        assert np.array_equal(rf.value[live], cpu.value[live])
        assert np.array_equal(rf.gain, cpu.gain)
        assert np.array_equal(rf.cover[live], cpu.cover[live])
    return rf, rep, (X, Y, F)


def assert_multi_block(rep, n, bootstrap, levels, nt):
    """Levels whose largest node takes several blocks, launched with nt threads."""
    for lv in levels:
        assert blocks(rep.max_rows[lv], lv) > 1, (lv, rep.max_rows)
        assert threads(n, bootstrap, lv) == nt, (lv, nt)


def test_thresholds_mirror_the_driver():
    """No GPU: the constants above are read back from csrc/forest.hip, so a retuning there fails here first and
    the path assertions below are revisited with it instead of going silently blind."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "forest.hip")).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, (pattern, m)
        return int(m[0])

    assert one(r"#define RF_CHUNK0 (\d+)") == RF_CHUNK0
    assert one(r"#define RF_CHUNK1 (\d+)") == RF_CHUNK1
    assert one(r"constexpr int RF_CHUNK = (\d+);") == RF_CHUNK
    assert one(r"constexpr int RF_BEGIN_LDS = (\d+);") == RF_BEGIN_LDS
    assert one(r"return \(kept >> level\) >= (\d+) \? RF_NT : 64;") == RF_SHAPE_NT_ROWS
    assert one(r"const int64_t b = N / (\d+);") == RF_SHAPE_BLOCK_ROWS
    assert one(r"constexpr int PB = (\d+);") * one(r"g0 \+= PB \* (\d+)\)") == RF_BEGIN_BATCH
    assert "level == 0 ? RF_CHUNK0 : (level == 1 ? RF_CHUNK1 : RF_CHUNK)" in src  # chunk() below


@gpu
def test_more_candidates_than_features_is_rejected():
    """k > F would leave candidate slots that are never filled: em_rf_fit refuses it before any launch."""
    from euromillioner_amd.ops import forest as K

    X = np.arange(1, 9, dtype=np.uint64).reshape(8, 1)
    Y = np.arange(8, 0, -1, dtype=np.uint64)
    with pytest.raises(ValueError, match="em_rf_fit"):
        K.fit(X, Y, 62, 0, 1, 1, 63, 1, False, 0)
    feat, _, _, cover = K.fit(X, Y, 62, 0, 1, 1, 62, 1, False, 0)  # k == F is the limit, and fits
    assert feat.shape == (1, 3) and cover[0, 0] == 8


# ------------------------------------------------------------------ multi-block nodes, fused record path
@gpu
@pytest.mark.parametrize("n,boot,depth,trees", [(40000, False, 6, 3), (70000, True, 6, 3), (40000, False, 7, 2)],
                         ids=["a-40000", "b-70000-boot", "c-depth7"])
def test_fused_multi_block_nodes(n, boot, depth, trees):
    """(c) is (a) one level deeper: the fused driver's last partition is at level max_depth - 2 (the last level's
    leaves come from their parents' split), so only at depth 7 does the 64-thread launch of level 5 really move a
    node of several blocks."""
    _, rep, (X, Y, F) = fit_and_check(Case("fused", ("draws", n, 1), depth, (0, trees), "sqrt", boot))
    assert row_bytes(X, F) == 16 and max_outputs(Y) <= 7  # position-form records
    assert rep.max_rows[0] > RF_CHUNK0 and listing_blocks(n) > 1
    assert_multi_block(rep, n, boot, range(1, 5), 256)
    assert rep.max_rows[5] > RF_CHUNK and threads(n, boot, 5) == 64


@gpu
def test_fused_multi_block_mask_form():
    n = 40000
    X, Y, _ = mask_form_data(n, 30)
    assert max_outputs(Y) > 7  # rf_ycheck: mask-form records
    _, rep, (X, Y, F) = fit_and_check(Case("mask", ("mask", n, 30), 3, (0, 3), "sqrt", False, seed=7))
    assert row_bytes(X, F) == 16
    assert rep.max_rows[0] == n and blocks(n, 0) > 1 and blocks(rep.max_rows[1], 1) > 1
    assert threads(n, False, 0) == 256 and threads(n, False, 1) == 256


@gpu
@pytest.mark.parametrize("n", [RF_CHUNK0, RF_CHUNK0 + 1])
def test_root_block_boundary(n):
    _, rep, _ = fit_and_check(Case("root", ("draws", n, 1), 2, (0, 2), "sqrt", False))
    assert rep.max_rows[0] == n and blocks(n, 0) == (1 if n == RF_CHUNK0 else 2)
    assert listing_blocks(n) == 8


# ------------------------------------------------------------------ multi-block nodes, index form
@gpu
def test_index_form_multi_block_nodes():
    n = 40000
    _, rep, (X, Y, F) = fit_and_check(Case("index", ("draws", n, 2), 4, (0, 2), "0.3", False))
    assert F == 124 and row_bytes(X, F) == 4
    assert rep.max_rows[0] > RF_CHUNK0 and listing_blocks(n) > 1
    assert_multi_block(rep, n, False, range(0, 4), 256)


@gpu
def test_index_form_64_threads_multi_block():
    """The opposite mix on the index-form kernels: bootstrap at 25000 rows makes level 3 a 64-thread
    launch (15800 / 8 < 2048) while the skewed draws still leave a node of more than RF_CHUNK rows."""
    n = 25000
    _, rep, (X, Y, F) = fit_and_check(Case("index64", ("draws", n, 2), 4, (0, 2), "0.3", True))
    assert row_bytes(X, F) == 4
    assert threads(n, True, 3) == 64 and blocks(rep.max_rows[3], 3) > 1


# ------------------------------------------------------------------ wide work lists
@gpu
@pytest.mark.parametrize("trees,depth,boot,n", [(100, 9, True, 2000), (40, 10, False, 1500)])
def test_wide_work_lists_fused(trees, depth, boot, n):
    _, rep, (X, Y, F) = fit_and_check(Case("wide", ("draws", n, 1), depth, (0, trees), "sqrt", boot))
    assert row_bytes(X, F) == 16
    last = depth - 1  # the last level rf_level_begin lists
    assert trees << last > RF_BEGIN_LDS and rep.max_flat[last] > RF_BEGIN_LDS
    assert rep.max_flat[last - 1] > RF_BEGIN_BATCH
    assert rep.reached[last] > 1000  # (not a lone straggler: a real level)


@gpu
def test_wide_work_lists_index_form():
    trees, depth, n = 72, 8, 2000
    _, rep, (X, Y, F) = fit_and_check(Case("wide-index", ("draws", n, 2), depth, (0, trees), "0.3", True))
    assert row_bytes(X, F) == 4
    # (rf_level_prep / rf_worklist list every level, the last included: 18 items per scan thread at level 8)
    assert rep.max_flat[depth] > RF_BEGIN_LDS and rep.max_flat[depth - 1] > RF_BEGIN_BATCH
    assert rep.reached[depth] > 1000


# ------------------------------------------------------------------ deep trees
@gpu
@pytest.mark.parametrize("depth,trees,n,boot,min_leaf", [(14, 2, 20000, False, 3), (12, 3, 20000, True, 1)])
def test_deep_trees(depth, trees, n, boot, min_leaf):
    _, rep, _ = fit_and_check(Case("deep", ("draws", n, 1), depth, (0, trees), "sqrt", boot, min_leaf))
    assert rep.reached[depth] > 0 and all(r > 0 for r in rep.reached)


# ------------------------------------------------------------------ the small cases, also against the numpy engine
_small = {}


@gpu
@pytest.mark.parametrize("case", SMALL_CASES, ids=repr)
def test_small_cases(case):
    rf, rep, (X, Y, F) = fit_and_check(case, compare_numpy=True)
    _small[case.name] = rf
    if case.name.startswith("dense"):
        assert row_bytes(X, F) == (16 if F == 62 else 4)
        assert (rf.feat[:, 0] >= 61).all()  # the planted bits
        if F > 62:
            assert (rf.feat >= 62).any()
    if case.name.startswith("lags"):
        assert X.shape[1] == (F + 63) // 64 and rf.k == n_candidates(case.subset, F)
    if case.name.startswith("y_zero"):
        assert (rf.feat[:, 0] == -1).all() and rep.nodes == len(case.trees)
    if case.name == "n1-boot":
        assert (rf.cover[:, 0] == 0).any() and not rf.value[rf.cover[:, 0] == 0].any()


@gpu
def test_device_shards_compose():
    """[0, 6) == [0, 3) ++ [3, 6) bit for bit on all four arrays (the tree id, not its position, is the key)."""
    by = {c.name: c for c in SMALL_CASES}
    parts = [_small.get(nm) or fit_and_check(by[nm])[0] for nm in ("shard0to3", "shard3to6")]
    full, _, _ = fit_and_check(Case("full", ("draws", 3000, 1), 5, (0, 6), "sqrt", True))
    for a in ("feat", "value", "gain", "cover"):
        whole, cat = getattr(full, a), np.concatenate([getattr(p, a) for p in parts])
        assert whole.tobytes() == cat.tobytes(), a
