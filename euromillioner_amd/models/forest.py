"""Random forest over binary draw features (BASELINE config 4).

The reference declares Spark MLlib (``pom.xml:56-61``) and advertises "Random Forest"
(``README.md:6``) but never builds one.  This is a multi-output forest: inputs are the
62-wide multi-hot of the current draw (``lags`` draws -> 62*lags features), outputs
the 62-wide multi-hot of the next draw; each leaf stores the weighted mean 62-vector.

Semantics (shared bit-for-bit by the HIP engine ``csrc/forest.hip`` and the numpy
oracle below):

* Poisson(1) bootstrap weights per (tree, row) from a counter hash (Spark's scheme);
* per-node candidate features: ``k`` of ``F`` by a hashed partial Fisher-Yates
  (``feature_subset``: sqrt | log2 | all | onethird | <fraction>, Spark's rounding: ceil);
* split gain = weighted variance reduction summed over the 62 outputs (== Gini/2 per
  output): ``SL2/nL + SR2/nR - S2/n`` from exact integer sums; a split needs both
  children to weigh ``>= min_samples_leaf`` and a gain above rounding noise;
* complete-array trees: node ``i`` -> children ``2i+1`` (feature = 0), ``2i+2`` (= 1).

Tree-parallel data parallelism (C5): rank r builds the trees ``shard_range(T)`` with
global tree ids (so the forest is identical for any world size) and the packed arrays
are all-gathered.
"""
from __future__ import annotations

import json
import math

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
POISSON_CDF = (0.36787944117144233, 0.7357588823428847, 0.9196986029286058, 0.9810118431238463,
               0.9963401531726563, 0.9994058151824183, 0.999916758850712, 0.9999897508033253, 0.999998874797402)
CAND_SALT = 0x5EEDF00D


def mix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hash3(seed, a, b):
    return mix64(mix64(np.uint64(seed) ^ mix64(a)) ^ np.asarray(b, dtype=np.uint64))


def poisson_weights(seed: int, tree: int, n: int) -> np.ndarray:
    h = hash3(seed, np.uint64((1 << 32) + tree), np.arange(n, dtype=np.uint64))
    u = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    w = np.zeros(n, dtype=np.int64)
    for c in POISSON_CDF:
        w += (u >= c)
    return w


def candidates(seed: int, tree: int, node: int, F: int, k: int) -> np.ndarray:
    arr = list(range(F))
    key = np.uint64((tree << 32) | node)
    s = np.uint64((seed ^ CAND_SALT) & 0xFFFFFFFFFFFFFFFF)
    hs = hash3(s, key, np.arange(min(k, F), dtype=np.uint64))  # (the stream does not depend on the swaps)
    for i in range(min(k, F)):
        j = i + int(hs[i]) % (F - i)
        arr[i], arr[j] = arr[j], arr[i]
    return np.array(arr[:min(k, F)], dtype=np.int64)


def n_candidates(strategy, F: int) -> int:
    s = str(strategy).lower()
    if s in ("all", "none"):
        return F
    if s in ("sqrt", "auto"):
        return max(1, math.ceil(math.sqrt(F)))
    if s == "log2":
        return max(1, math.ceil(math.log2(F)))
    if s == "onethird":
        return max(1, math.ceil(F / 3))
    frac = float(s)
    if not 0 < frac <= 1:
        raise ValueError(f"feature_subset fraction must be in (0, 1], got {strategy}")
    return max(1, math.ceil(frac * F))


def pack_bits(B: np.ndarray) -> np.ndarray:
    """[N, F] {0,1} -> [N, ceil(F/64)] uint64 (feature f = bit f%64 of word f//64)."""
    B = np.asarray(B).astype(bool)
    n, F = B.shape
    W = max(1, (F + 63) // 64)
    out = np.zeros((n, W), dtype=np.uint64)
    for f in range(F):
        out[:, f // 64] |= B[:, f].astype(np.uint64) << np.uint64(f % 64)
    return out


def unpack_bits(Xw: np.ndarray, F: int) -> np.ndarray:
    Xw = np.asarray(Xw, dtype=np.uint64).reshape(len(Xw), -1)
    out = np.zeros((len(Xw), F), dtype=np.int64)
    for f in range(F):
        out[:, f] = ((Xw[:, f // 64] >> np.uint64(f % 64)) & np.uint64(1)).astype(np.int64)
    return out


def draw_features(numbers: np.ndarray, lags: int = 1) -> tuple[np.ndarray, np.ndarray, int]:
    """Draw rows -> (X bits [S, W], Y masks [S], F) for samples t = lags-1 .. N-2."""
    from ..data.draws import lag_features, mask_bits

    if lags == 1:
        m = mask_bits(numbers)
        return m[:-1].reshape(-1, 1).copy(), m[1:].copy(), 62
    X, Y = lag_features(numbers, lags)
    return pack_bits(X), pack_bits(Y)[:, 0].copy(), 62 * lags


class RandomForest:
    def __init__(self, n_trees: int = 100, max_depth: int = 8, min_samples_leaf: int = 1,
                 feature_subset="sqrt", bootstrap: bool = True, seed: int = 0, device: str = "auto"):
        if not 0 <= max_depth <= 14:
            raise ValueError("max_depth must be in [0, 14] (complete-array trees)")
        if n_trees < 1 or min_samples_leaf < 1:
            raise ValueError("n_trees and min_samples_leaf must be >= 1")
        self.n_trees, self.max_depth, self.min_samples_leaf = int(n_trees), int(max_depth), int(min_samples_leaf)
        self.feature_subset, self.bootstrap, self.seed, self.device = feature_subset, bool(bootstrap), int(seed), device
        self.nodes = (1 << (max_depth + 1)) - 1
        self.F = None
        self.feat = self.value = self.gain = self.cover = None
        self.backend_used = None
        self.n_train = None  # rows of the last fit (None: unknown, e.g. an older forest file)
        self.tree_start = 0  # global id of tree 0 (fit with an explicit trees= range)
        self.explain_backend_used = None  # numpy | hip: what the last predict_contribs / apply ran on

    # ------------------------------------------------------------------ fit
    def _backend(self) -> str:
        if self.device == "cpu":
            return "numpy"
        try:
            import torch

            if torch.cuda.is_available():
                return "hip"
        except Exception:  # noqa: BLE001
            pass
        if self.device == "cuda":
            raise RuntimeError("device=cuda requested but no GPU is available")
        return "numpy"

    def fit(self, X: np.ndarray, Y: np.ndarray, F: int, trees: range | None = None, group=None) -> "RandomForest":
        """X: [N, W] uint64 feature bits, Y: [N] uint64 target masks (bits 0..61), F features."""
        X = np.ascontiguousarray(np.asarray(X, dtype=np.uint64).reshape(len(X), -1))
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.uint64).reshape(-1))
        if F > 64 * X.shape[1] or F > 256:
            raise ValueError("F exceeds the packed feature words (max 256)")
        self.F = int(F)
        self.k = n_candidates(self.feature_subset, F)
        self.n_train = len(X)
        self.tree_start = int(trees.start) if trees is not None and group is None else 0
        if trees is None:
            trees = range(self.n_trees)
            if group is not None:
                from ..parallel.dist import shard_range, DistInfo
                import torch.distributed as dist

                info = DistInfo(dist.get_rank(group), dist.get_world_size(group))
                a, b = shard_range(self.n_trees, info)
                trees = range(a, b)
        be = self._backend()
        self.backend_used = be
        if be == "hip":
            feat, value, gain, cover = self._fit_hip(X, Y, trees)
        else:
            feat, value, gain, cover = self._fit_numpy(X, Y, trees)
        if group is not None:
            feat, value, gain, cover = self._gather(group, trees, feat, value, gain, cover)
        self.feat, self.value, self.gain, self.cover = feat, value, gain, cover
        return self

    def fit_draw_masks(self, masks, lags: int = 1, rows: tuple[int, int] | None = None, group=None):
        """Fit on device draw masks (int64 [n] on the GPU): samples ``rows = (a, b)`` of the lag-window numbering of
        ``ops.tree_inputs.rf_rows`` (sample ``s``: draws ``s .. s+lags-1`` -> draw ``s+lags``; default: all of
        them).  The packed rows are built on the device and never leave it; the trees equal :meth:`fit` on the
        host rows ``draw_features`` builds from the same draws.  Single process."""
        if group is not None:
            raise ValueError("fit_draw_masks is single-process (no process group)")
        if self.device == "cpu":
            raise ValueError("fit_draw_masks runs on the GPU (device=cpu was asked for)")
        from ..ops import forest as K
        from ..ops import tree_inputs as TI

        a, b = (0, None) if rows is None else (int(rows[0]), int(rows[1]))
        X, Y, F = TI.rf_rows(masks, lags, first=a, count=None if b is None else b - a)
        self.F = int(F)
        self.k = n_candidates(self.feature_subset, F)
        self.n_train = int(X.shape[0])
        self.tree_start = 0
        self.backend_used = "hip"
        self.feat, self.value, self.gain, self.cover = K.fit(
            X, Y, self.F, 0, self.n_trees, self.max_depth, self.k, self.min_samples_leaf, self.bootstrap, self.seed,
            device=masks.device)
        return self

    def _fit_numpy(self, X, Y, trees):
        from .forest_oracle import grow_forest_numpy

        return grow_forest_numpy(X, Y, self.F, list(trees), self.max_depth, self.k, self.min_samples_leaf,
                                 self.bootstrap, self.seed)

    def _fit_hip(self, X, Y, trees):
        import torch

        from ..ops import forest as K

        return K.fit(X, Y, self.F, trees.start, len(trees), self.max_depth, self.k, self.min_samples_leaf,
                     self.bootstrap, self.seed)

    def _gather(self, group, trees, feat, value, gain, cover):
        """C5: all-gather the packed per-rank tree arrays (tree ids are global, so order is fixed)."""
        import torch.distributed as dist

        parts = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, (trees.start, feat, value, gain, cover), group=group)
        parts.sort(key=lambda p: p[0])
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(1, 5))

    # ------------------------------------------------------------------ predict
    def predict_proba(self, X: np.ndarray) -> np.ndarray:
        """[N, 62] mean leaf vector over trees (numpy traversal)."""
        X = np.asarray(X, dtype=np.uint64).reshape(len(X), -1)
        n = len(X)
        bits = unpack_bits(X, self.F)
        acc = np.zeros((n, 64), dtype=np.float64)
        rows = np.arange(n)
        for t in range(len(self.feat)):
            node = np.zeros(n, dtype=np.int64)
            for _ in range(self.max_depth + 1):
                f = self.feat[t][node]
                act = f >= 0
                if not act.any():
                    break
                b = bits[rows[act], f[act]]
                node[act] = 2 * node[act] + 1 + b
            acc += self.value[t][node]
        return (acc / max(len(self.feat), 1))[:, :62].astype(np.float32)

    def predict_proba_device(self, X, out_logit: bool = False):
        """Same on the GPU (K11): returns a [N, 64] fp32 device tensor."""
        from ..ops import forest as K

        return K.predict(X, self.feat, self.value, self.max_depth, out_logit=out_logit)

    # ------------------------------------------------------------------ out-of-bag evaluation, importances
    def _oob_device(self, X):
        from ..ops import forest as K
        from .forest_oob import check_oob_args

        X = check_oob_args(self, X)
        return K.oob_predict(X, self.feat, self.value, self.max_depth, self.seed, self.tree_start)

    def oob_predict_proba(self, X: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """(proba [N, 62] float32, count [N] int32): per training row the mean leaf vector over the trees it
        is out of bag for (bootstrap weight 0) and their number.  ``X`` must be the matrix of the fit, same
        rows in the same order: the row index is the hash key.  Definitions: ``models/forest_oob.py``."""
        from .forest_oob import oob_predict_proba_numpy

        if self._backend() == "hip":
            out, count = self._oob_device(X)
            return out[:, :62].cpu().numpy(), count.cpu().numpy()
        return oob_predict_proba_numpy(self, X)

    def oob_score(self, X: np.ndarray, Y: np.ndarray) -> dict:
        """The forest's out-of-bag score on its training rows (X as ``oob_predict_proba``, Y [N] target masks):
        rows, rows_without_oob_tree, min_trees, mean_trees, hits_main, hits_star, exact, acc, trivial_acc,
        brier, logloss over the rows with at least one out-of-bag tree."""
        from .forest_oob import oob_finish, oob_predict_proba_numpy, oob_totals_numpy

        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.uint64).reshape(-1))
        if len(Y) != len(X):
            raise ValueError("X and Y row counts differ")
        if self._backend() == "hip":
            from ..ops import forest as K

            out, count = self._oob_device(X)
            return K.oob_metrics(out, count, Y)
        proba, count = oob_predict_proba_numpy(self, X)
        return oob_finish(oob_totals_numpy(proba, count, Y))

    def feature_importances(self, kind: str = "gain") -> np.ndarray:
        """[F] float64 shares of the split nodes' gain | cover | splits per feature (sum 1; zeros without a split)."""
        from .forest_oob import feature_importances

        return feature_importances(self, kind)

    # ------------------------------------------------------------------ explanations (models/forest_explain.py)
    def _explain_backend(self, backend, need_plan: bool) -> str:
        """numpy | hip for an explanation call.  ``None``: HIP when a GPU is present (and, for contributions,
        the forest is inside the device plan), else numpy.  ``"hip"`` outside the plan raises."""
        if backend not in (None, "numpy", "hip"):
            raise ValueError(f"backend must be None, 'numpy' or 'hip', got {backend!r}")
        if backend == "numpy":
            return "numpy"
        if backend is None and self._backend() != "hip":
            return "numpy"
        if need_plan:
            from ..ops import forest as K

            if not K.shap_plan(self.F, self.max_depth):
                if backend == "hip":
                    raise ValueError(f"GPU TreeSHAP: no plan for max_depth {self.max_depth} with {self.F} features "
                                     f"(the plan covers max_depth <= 8 and F <= 256)")
                return "numpy"
        return "hip"

    def _shap_tables(self):
        """The device path table (em_rf_shap_paths), built once per fitted forest."""
        from ..ops import forest as K
        from . import forest_explain as E

        cached = getattr(self, "_shap_device", None)
        if cached is not None and cached[0] is self.feat:
            return cached[1]
        E.paths_of(self)  # validates on the host: the kernels index by feat and assume distinct path features
        tables = K.shap_tables(self.feat, self.value, self.cover, E.leaf_mask(self.feat), self.max_depth, self.F)
        self._shap_device = (self.feat, tables)
        return tables

    def _check_rows(self, X):
        if self.feat is None:
            raise ValueError("the forest is not fitted")
        X = np.asarray(X, dtype=np.uint64).reshape(len(X), -1)
        W = (self.F + 63) // 64
        if X.shape[1] < W:
            raise ValueError(f"X has {X.shape[1]} feature words, the forest needs {W}")
        return np.require(X[:, :W], requirements=["C", "W"])  # (a read-only input is copied: torch wants writable)

    def predict_contribs_device(self, X):
        """:meth:`predict_contribs` on the GPU, as a [n, 62, F+1] fp32 device tensor (no host copy, no chunks)."""
        from ..ops import forest as K

        self.explain_backend_used = self._explain_backend("hip", need_plan=True)
        return K.shap(self._check_rows(X), self._shap_tables())

    def predict_contribs(self, X: np.ndarray, backend: str | None = None, chunk_rows: int | None = None) -> np.ndarray:
        """float32 ``[n, 62, F+1]`` path-dependent TreeSHAP contributions of :meth:`predict_proba` on packed rows
        ``X`` [n, W], the bias (the forest's expectation under its covers) in the last column:
        ``phi[r, o, :F].sum() + phi[r, o, F] == predict_proba[r, o]`` up to rounding.  ``backend``: None | numpy |
        hip.  On the GPU the rows go through the kernel ``chunk_rows`` at a time; a row's result depends on the
        row only."""
        from . import forest_explain as E

        X = self._check_rows(X)
        self.explain_backend_used = self._explain_backend(backend, need_plan=True)
        if self.explain_backend_used == "numpy":
            return E.contribs_numpy(self, X).astype(np.float32)
        from ..ops import forest as K

        tables = self._shap_tables()
        n, row_bytes = len(X), 62 * (self.F + 1) * 4
        if chunk_rows is None:
            chunk_rows = max(256, (256 << 20) // row_bytes)
        chunk_rows = int(chunk_rows)
        if chunk_rows < 1:
            raise ValueError("chunk_rows must be positive")
        out = np.empty((n, 62, self.F + 1), dtype=np.float32)
        for a in range(0, n, chunk_rows):
            out[a:a + chunk_rows] = K.shap(X[a:a + chunk_rows], tables).cpu().numpy()
        return out

    def apply(self, X: np.ndarray, backend: str | None = None) -> np.ndarray:
        """int32 ``[n, T]``: the heap index of the leaf each row stops at in each tree (sklearn's ``apply``)."""
        from . import forest_explain as E

        X = self._check_rows(X)
        self.explain_backend_used = self._explain_backend(backend, need_plan=False)
        if self.explain_backend_used == "numpy":
            return E.apply_numpy(self, X)
        from ..ops import forest as K

        E.paths_of(self)  # (validation: the kernel indexes the row's words by feat)
        if len(X) == 0:
            return np.zeros((0, len(self.feat)), dtype=np.int32)
        return K.leaf_index(X, self.feat, self.max_depth, self.F).cpu().numpy()

    # ------------------------------------------------------------------ persistence (T6 tree file)
    def meta(self) -> dict:
        return {"format": "euromillioner-forest-v1", "n_trees": len(self.feat), "max_depth": self.max_depth,
                "min_samples_leaf": self.min_samples_leaf, "feature_subset": str(self.feature_subset),
                "bootstrap": self.bootstrap, "seed": self.seed, "F": self.F, "k": self.k,
                "n_train": self.n_train, "tree_start": self.tree_start}

    def save(self, path: str) -> None:
        """``.npz`` of plain arrays + JSON meta (loadable with allow_pickle=False)."""
        np.savez(path, feat=self.feat, value=self.value, gain=self.gain, cover=self.cover,
                 meta=np.frombuffer(json.dumps(self.meta()).encode(), dtype=np.uint8))

    @classmethod
    def load(cls, path: str) -> "RandomForest":
        z = np.load(path, allow_pickle=False)
        meta = json.loads(bytes(z["meta"]).decode())
        if meta.get("format") != "euromillioner-forest-v1":
            raise ValueError("not a forest file")
        rf = cls(meta["n_trees"], meta["max_depth"], meta["min_samples_leaf"], meta["feature_subset"],
                 meta["bootstrap"], meta["seed"])
        rf.F, rf.k = meta["F"], meta["k"]
        rf.n_train, rf.tree_start = meta.get("n_train"), int(meta.get("tree_start", 0))  # (absent in older files)
        rf.feat, rf.value, rf.gain, rf.cover = z["feat"], z["value"], z["gain"], z["cover"]
        return rf
