"""Python face of the random-forest kernels (``csrc/forest.hip``: K8 hist, K9 split scan,
K10 partition, K11 predict, K11-OOB out-of-bag predict and metrics) and their native level-wise driver ``em_rf_fit``,
and of the explanation kernels (``csrc/forest_shap.hip``: TreeSHAP contributions, leaf indices).

The reference only declares Spark MLlib's RandomForest (``/root/reference/pom.xml:56-61``,
``README.md:6``); SURVEY.md §2.4 N7 / BASELINE config 4 define the 100-tree one-hot forest."""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N

N.register_signatures({
    "em_rf_nodes": (N._i32, [N._i32]),
    "em_rf_row_bytes": (N._i32, [N._i32, N._i32, N._i64]),
    "em_rf_acc_words": (N._i64, [N._i32, N._i32, N._i32]),
    "em_rf_fit": (N._i32, [N._c_void_p, N._i32, N._c_void_p, N._i64, N._i32, N._i32, N._i32, N._i32, N._i32, N._i32,
                           N.ctypes.c_uint64, N._i32, N._c_void_p, N._c_void_p, N._c_void_p, N._c_void_p, N._c_void_p,
                           N._c_void_p, N._c_void_p, N._c_void_p, N._c_void_p, N._c_void_p, N._c_void_p,
                           N._c_void_p]),
    "em_rf_predict": (N._i32, [N._c_void_p, N._i32, N._i64, N._c_void_p, N._c_void_p, N._i32, N._i32, N._i32,
                               N._c_void_p, N._i32, N._c_void_p, N._c_void_p]),
    "em_rf_predict_scratch": (N._i64, [N._i32, N._i32, N._i32]),
    "em_rf_oob_predict": (N._i32, [N._c_void_p, N._i32, N._i64, N._c_void_p, N._c_void_p, N._i32, N._i32,
                                   N.ctypes.c_uint64, N._i32, N._c_void_p, N._i32, N._c_void_p, N._c_void_p,
                                   N._c_void_p]),
    "em_rf_oob_metrics_words": (N._i64, [N._i64]),
    "em_rf_oob_metrics": (N._i32, [N._c_void_p, N._i32, N._c_void_p, N._c_void_p, N._i64, N._c_void_p, N._c_void_p]),
    "em_rf_shap_lds_bytes": (N._i32, [N._i32, N._i32]),
    "em_rf_shap_paths": (N._i32, [N._i32, N._i32, N._i32, N._i32] + [N._c_void_p] * 11),
    "em_rf_shap": (N._i32, [N._c_void_p, N._i32, N._i32, N._i32, N._i32, N._i32, N._i32] + [N._c_void_p] * 7),
    "em_rf_leaf_index": (N._i32, [N._c_void_p, N._i32, N._i64, N._i32, N._c_void_p, N._i32, N._i32, N._c_void_p,
                                  N._c_void_p]),
})


def _u64_to_device(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(device)


def fit(X: np.ndarray | torch.Tensor, Y: np.ndarray | torch.Tensor, F: int, t_off: int, T: int, max_depth: int,
        k: int, min_leaf: int, bootstrap: bool, seed: int, device="cuda", return_device: bool = False):
    """Grow trees [t_off, t_off+T) on the GPU; returns (feat, value, gain, cover) numpy arrays."""
    dev = torch.device(device)
    Xd = X if isinstance(X, torch.Tensor) else _u64_to_device(X, dev)
    Yd = Y if isinstance(Y, torch.Tensor) else _u64_to_device(Y, dev)
    n = Xd.shape[0]
    W = Xd.shape[1] if Xd.dim() == 2 else 1
    if Yd.numel() != n:
        raise ValueError("X and Y row counts differ")
    if n >= 2**31 - 1 or n < 1:
        raise ValueError("rows must be in [1, 2^31-2]")
    nodes = (1 << (max_depth + 1)) - 1
    # per-tree row lists: 16-B records (x, y, weight) for one-word features, else int32 row ids
    rw = N.query("em_rf_row_bytes", W, F, n) // 4
    rows_a = torch.empty(T, n, rw, dtype=torch.int32, device=dev)
    rows_b = torch.empty(T, n, rw, dtype=torch.int32, device=dev)
    seg = torch.empty(T, nodes, 2, dtype=torch.int32, device=dev)
    feat = torch.full((T, nodes), -2, dtype=torch.int16, device=dev)
    value = torch.zeros(T, nodes, 64, dtype=torch.float32, device=dev)
    gain = torch.zeros(T, nodes, dtype=torch.float64, device=dev)
    cover = torch.zeros(T, nodes, dtype=torch.float32, device=dev)
    # per-level scratch: candidate lists, per-node integer sums, partition counters
    acc_words = N.query("em_rf_acc_words", T, max_depth, k)
    if acc_words < 0:
        raise ValueError("unsupported forest shape (trees / depth / candidate count)")
    cand = torch.empty(T, 1 << max_depth, k, dtype=torch.int16, device=dev)
    acc = torch.empty(acc_words, dtype=torch.int32, device=dev)
    lrc = torch.empty(T, 1 << max_depth, 2, dtype=torch.int32, device=dev)
    wl = torch.empty(T * (1 << max_depth) + 1, dtype=torch.int32, device=dev)  # per-level work list
    N.call("em_rf_fit", Xd.data_ptr(), W, Yd.data_ptr(), n, F, T, max_depth, k, min_leaf, int(bootstrap),
           int(seed) & 0xFFFFFFFFFFFFFFFF, int(t_off), rows_a.data_ptr(), rows_b.data_ptr(), seg.data_ptr(),
           feat.data_ptr(), value.data_ptr(), gain.data_ptr(), cover.data_ptr(), cand.data_ptr(), acc.data_ptr(),
           lrc.data_ptr(), wl.data_ptr(), N.stream_handle(dev))
    del rows_a, rows_b, cand, acc, lrc, wl
    if return_device:
        return feat, value, gain, cover
    return feat.cpu().numpy(), value.cpu().numpy(), gain.cpu().numpy(), cover.cpu().numpy()


def fit_buffer_bytes(n: int, W: int, F: int, T: int, max_depth: int, k: int) -> int:
    """Device bytes :func:`fit` allocates for ``T`` trees on ``n`` rows of ``W`` words (the rows X [n, W] and the
    targets Y [n] included): the shapes above, for a check against the free memory before a large fit."""
    nodes, half = (1 << (max_depth + 1)) - 1, 1 << max_depth
    acc_words = N.query("em_rf_acc_words", T, max_depth, k)
    if acc_words < 0:
        raise ValueError("unsupported forest shape (trees / depth / candidate count)")
    row_lists = 2 * T * n * N.query("em_rf_row_bytes", W, F, n)
    trees = T * nodes * (2 * 4 + 2 + 64 * 4 + 8 + 4)  # seg, feat, value, gain, cover
    scratch = T * half * k * 2 + acc_words * 4 + T * half * 2 * 4 + (T * half + 1) * 4  # cand, acc, lrc, wl
    return int(8 * n * (W + 1) + row_lists + trees + scratch)


def _predict_args(X, feat, value, max_depth: int, stream_trees: bool, device):
    """What predict and oob_predict share: X, feat and value on the device, the shape check, ``out`` [N, 64] and
    the tree-image scratch.  Returns the leading arguments of either entry point (X, W, N, feat, value, T,
    max_depth), ``out``, the scratch pointer (None: one wave per row), the stream, and the tensors behind the
    pointers for the caller to hold until its launch is queued."""
    dev = torch.device(device)
    Xd = X if isinstance(X, torch.Tensor) else _u64_to_device(X, dev)
    n = Xd.shape[0]
    W = Xd.shape[1] if Xd.dim() == 2 else 1
    fd = feat if isinstance(feat, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(feat)).to(dev)
    vd = value if isinstance(value, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(value)).to(dev)
    T = fd.shape[0]
    if fd.shape[1] != (1 << (max_depth + 1)) - 1:
        raise ValueError("feat does not match max_depth")
    out = torch.empty(n, 64, dtype=torch.float32, device=dev)
    nb = N.lib().em_rf_predict_scratch(W, T, max_depth) if stream_trees else 0
    prep = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev) if nb > 0 else None
    head = (Xd.data_ptr(), W, n, fd.data_ptr(), vd.data_ptr(), T, max_depth)
    return head, out, prep.data_ptr() if prep is not None else None, N.stream_handle(dev), (Xd, fd, vd, prep)


def predict(X, feat, value, max_depth: int, out_logit: bool = False, device="cuda", stream_trees: bool = True
            ) -> torch.Tensor:
    """K11: mean leaf vector per row -> [N, 64] fp32 (probabilities, or logits if out_logit).
    ``stream_trees``: single-word rows and depth <= 8 stream the trees through LDS (csrc/forest.hip
    rf_predict_lds, bit-identical); False forces the one-wave-per-row kernel."""
    head, out, prep, st, _keep = _predict_args(X, feat, value, max_depth, stream_trees, device)
    N.call("em_rf_predict", *head, int(out_logit), out.data_ptr(), 64, prep, st)
    return out


def oob_predict(X, feat, value, max_depth: int, seed: int, t_off: int = 0, stream_trees: bool = True, device="cuda"
                ) -> tuple[torch.Tensor, torch.Tensor]:
    """K11-OOB: per row the mean leaf vector over the trees it is out of bag for -> (out [N, 64] fp32, count [N]
    int32).  ``X`` must be the matrix trees ``t_off .. t_off + T - 1`` (global ids) were fitted on with ``seed``:
    the in-bag sets are recomputed from the hash of (seed, tree id, row).  Rows without an out-of-bag tree are
    all zero with count 0.  ``stream_trees`` as :func:`predict` (rf_predict_lds<G, OOB>, bit-identical)."""
    head, out, prep, st, _keep = _predict_args(X, feat, value, max_depth, stream_trees, device)
    count = torch.empty(out.shape[0], dtype=torch.int32, device=out.device)
    N.call("em_rf_oob_predict", *head, int(seed) & 0xFFFFFFFFFFFFFFFF, int(t_off), out.data_ptr(), 64,
           count.data_ptr(), prep, st)
    return out, count


def oob_totals(out: torch.Tensor, count: torch.Tensor, Y) -> dict:
    """em_rf_oob_metrics: the per-block partials of the rows with count > 0, added on the host in block order
    (integers exactly, the fp64 Brier / log-loss sums one block after the other).  Keys as
    ``models.forest_oob.oob_totals_numpy``."""
    from ..models.forest_oob import TOTAL_KEYS

    N.check_cuda(out, "out", torch.float32)
    N.check_cuda(count, "count", torch.int32)
    n = out.shape[0]
    if out.dim() != 2 or out.shape[1] < 62 or count.numel() != n:
        raise ValueError("out must be [N, >= 62] and count [N]")
    Yd = Y if isinstance(Y, torch.Tensor) else _u64_to_device(np.asarray(Y).reshape(-1), out.device)
    if Yd.numel() != n:
        raise ValueError("Y and out row counts differ")
    words = N.query("em_rf_oob_metrics_words", n)
    part = torch.empty(max(words, 1), dtype=torch.int64, device=out.device)
    N.call("em_rf_oob_metrics", out.data_ptr(), out.stride(0), count.data_ptr(), Yd.data_ptr(), n, part.data_ptr(),
           N.stream_handle(out.device))
    p = part[:words].cpu().numpy().reshape(-1, 10)
    tot = {k: int(p[:, i].sum()) for i, k in enumerate(TOTAL_KEYS[:8]) if k != "min_trees"}
    tot["min_trees"] = int(p[:, 6].min()) if len(p) and tot["rows"] > 0 else 0
    fl = p[:, 8:].copy().view(np.float64)
    tot["brier_sum"] = float(np.cumsum(fl[:, 0])[-1]) if len(p) else 0.0  # (cumsum: strictly in block order)
    tot["logloss_sum"] = float(np.cumsum(fl[:, 1])[-1]) if len(p) else 0.0
    tot["n"] = int(n)
    return tot


def oob_metrics(out: torch.Tensor, count: torch.Tensor, Y) -> dict:
    """The out-of-bag score of (out, count) = :func:`oob_predict` against the target masks ``Y`` [N]."""
    from ..models.forest_oob import oob_finish

    return oob_finish(oob_totals(out, count, Y))


# ----------------------------------------------------------------------------- explanations (csrc/forest_shap.hip)
class ShapTables:
    """The device leaf-path table of a forest (em_rf_shap_paths) and its bias row."""

    def __init__(self, T, L, max_depth, F, pd, pf, pz, pval, bias):
        self.T, self.L, self.max_depth, self.F = T, L, max_depth, F
        self.pd, self.pf, self.pz, self.pval, self.bias = pd, pf, pz, pval, bias


def shap_plan(F: int, max_depth: int) -> bool:
    """Whether the contribution kernel covers the shape (max_depth <= 8, F <= 256)."""
    return N.query("em_rf_shap_lds_bytes", int(F), int(max_depth)) >= 0


def shap_tables(feat: np.ndarray, value: np.ndarray, cover: np.ndarray, leaves: np.ndarray, max_depth: int, F: int,
                device="cuda") -> ShapTables:
    """Build the path table of a validated forest on the device.  ``leaves`` is the bool [T, nodes] mask of its
    leaves (``forest_explain.leaf_mask``): the host fixes each leaf's place in the table, the kernel fills it."""
    dev = torch.device(device)
    T, NN = feat.shape
    leaves = np.asarray(leaves, dtype=bool)
    L = int(leaves.sum())
    slot = np.where(leaves.reshape(-1), np.cumsum(leaves.reshape(-1)) - 1, -1).astype(np.int32)
    S = max(1, int(max_depth))
    d_slot = torch.from_numpy(slot).to(dev)
    fd = torch.from_numpy(np.ascontiguousarray(feat, dtype=np.int16)).to(dev)
    vd = torch.from_numpy(np.ascontiguousarray(value, dtype=np.float32)).to(dev)
    cd = torch.from_numpy(np.ascontiguousarray(cover, dtype=np.float32)).to(dev)
    pd = torch.empty(L, dtype=torch.int32, device=dev)
    pf = torch.empty(L, dtype=torch.int64, device=dev)  # 8 feature bytes per leaf
    pz = torch.empty(L * S, dtype=torch.float32, device=dev)
    pval = torch.empty(L, 64, dtype=torch.float32, device=dev)
    pbias = torch.empty(L, 64, dtype=torch.float64, device=dev)
    bias = torch.empty(64, dtype=torch.float32, device=dev)
    N.call("em_rf_shap_paths", T, int(max_depth), int(F), L, d_slot.data_ptr(), fd.data_ptr(), vd.data_ptr(),
           cd.data_ptr(), pd.data_ptr(), pf.data_ptr(), pz.data_ptr(), pval.data_ptr(), pbias.data_ptr(),
           bias.data_ptr(), N.stream_handle(dev))
    torch.cuda.synchronize(dev)  # (the inputs and pbias are released here)
    return ShapTables(T, L, int(max_depth), int(F), pd, pf, pz, pval, bias)


def shap(X, tables: ShapTables, out: torch.Tensor | None = None) -> torch.Tensor:
    """em_rf_shap: [n, 62, F+1] fp32 contributions (bias last) of packed rows ``X`` [n, W] on the device."""
    dev = tables.pd.device
    Xd = X if isinstance(X, torch.Tensor) else _u64_to_device(np.asarray(X).reshape(len(X), -1), dev)
    n = Xd.shape[0]
    W = Xd.shape[1] if Xd.dim() == 2 else 1
    if out is None:
        out = torch.empty(n, 62, tables.F + 1, dtype=torch.float32, device=dev)
    elif out.shape != (n, 62, tables.F + 1) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 [n, 62, F+1]")
    N.call("em_rf_shap", Xd.data_ptr(), W, n, tables.F, tables.max_depth, tables.T, tables.L, tables.pd.data_ptr(),
           tables.pf.data_ptr(), tables.pz.data_ptr(), tables.pval.data_ptr(), tables.bias.data_ptr(), out.data_ptr(),
           N.stream_handle(dev))
    return out


def leaf_index(X, feat, max_depth: int, F: int, device="cuda") -> torch.Tensor:
    """em_rf_leaf_index: [n, T] int32 heap index of the node each row stops at in each tree."""
    dev = torch.device(device)
    Xd = X if isinstance(X, torch.Tensor) else _u64_to_device(np.asarray(X).reshape(len(X), -1), dev)
    n = Xd.shape[0]
    W = Xd.shape[1] if Xd.dim() == 2 else 1
    fd = feat if isinstance(feat, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(feat, dtype=np.int16)).to(dev)
    T = fd.shape[0]
    if fd.shape[1] != (1 << (max_depth + 1)) - 1:
        raise ValueError("feat does not match max_depth")
    out = torch.empty(n, T, dtype=torch.int32, device=dev)
    N.call("em_rf_leaf_index", Xd.data_ptr(), W, n, int(F), fd.data_ptr(), T, int(max_depth), out.data_ptr(),
           N.stream_handle(dev))
    return out
