"""Device side of :mod:`euromillioner_amd.models.gbdt`: buffers + calls into ``csrc/gbdt.hip``.

Replaces the reference's ``XGBoost.train`` / ``Booster.predict`` JNI calls
(``/root/reference/src/main/java/com/euromillioner/Main.java:136-141``):
all rounds and levels run on the stream from the native driver ``em_gbdt_fit``; under data
parallelism (C4) the per-level histogram is all-reduced between the hist and split kernels."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ..ops import _native as N
from .gbdt import TreeArrays, apply_bins, quant_bits

_v, _i, _i64, _f, _u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint32


class _Eval(ctypes.Structure):
    _fields_ = [("bins", _v), ("Y", _v), ("margin", _v), ("n", _i)]


N.register_signatures({
    "em_gbdt_fit": (_i, [_v, _v, _i, _i, _v, _v, _i, _v, ctypes.POINTER(_Eval), _i, _i, _i, _i, _i, _i, _f, _f, _f,
                         _f, _f, _u32, _v, _v, _v, _v, _v, _i64, _v, _v, _v, _v, _v, _v, _v, _v, _v, _v, _i, _i, _v]),
    "em_gbdt_partial_doubles": (_i64, [_i, _i, _i, _v, _i]),
    "em_gbdt_init_margin": (_i, [_v, _i64, _f, _v]),
    "em_gbdt_predict": (_i, [_v, _v, _i, _i, _i, _i, _i, _i, _v, _v, _v, _v, _v]),
    "em_gbdt_dp_round_begin": (_i, [_i, _i, _i, _i, _v, _v, _v, _v, _v, _i, _f, _u32, _v, _v, _v, _v, _v]),
    "em_gbdt_dp_level_hist": (_i, [_i, _v, _v, _v, _v, _i, _i, _i, _v, _v, _v, _i64, ctypes.POINTER(_i64), _v]),
    "em_gbdt_dp_level_split": (_i, [_i, _v, _v, _i, _i, _i, _v, _i, _i, _v, _v, _v, _v, _v, _v, _v, _f, _f, _v]),
    "em_gbdt_dp_round_end": (_i, [_i, _i, _i, _v, _v, _v, _v, _v, _v, _v, _v, _v, _f, _f, _f, _v]),
    "em_gbdt_metric_sum": (_i, [_v, _v, _i, _i, _i, _i, _v, _v, _v]),
    # csrc/gbdt_shap.hip
    "em_gbdt_shap_lds_bytes": (_i, [_i, _i]),
    "em_gbdt_shap_paths": (_i, [_i, _i, _i, _v, _v, _v, _v, _v, _v, _v, _v, _v, _v, _v, _v, _v]),
    "em_gbdt_shap": (_i, [_v, _i, _i, _i, _i, _i, _i, _i, ctypes.c_double, _v, _v, _v, _v, _v, _v, _v, _v, _v, _v]),
    "em_gbdt_leaf_index": (_i, [_v, _v, _i, _i, _i, _i, _v, _v, _v, _v]),
})

OBJ = {"reg:logistic": 0, "binary:logistic": 0, "reg:squarederror": 1, "multi:softprob": 2, "multi:softmax": 2}
MET = {"logloss": 0, "rmse": 1, "error": 2, "mlogloss": 3, "merror": 4}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


class PlanUnsupported(ValueError):
    """The device engine has no histogram plan for this shape (per-level histograms too large)."""


class _Cells:
    """Compact histogram axis: feature f owns bins [off[f], off[f+1]) (host array for the native
    tile planner, device copy for the kernels)."""

    def __init__(self, cuts, dev):
        nbf = np.array([len(c) + 1 for c in cuts], dtype=np.int64)
        if (nbf > 256).any():
            raise PlanUnsupported("GPU GBDT supports at most 256 bins per feature")
        self.host = np.ascontiguousarray(np.concatenate([[0], np.cumsum(nbf)]).astype(np.int32))
        self.dev = torch.from_numpy(self.host).to(dev)
        self.C = int(self.host[-1])

    @property
    def hp(self):
        return self.host.ctypes.data


def fit(model, X, bins, nbins, Y, evals, rounds_per_call: int = 500, dp=None):
    """Returns (trees, history).  ``model.train_history`` gets the eval metric on the training rows after
    each round (R floats, column 0 of the driver's per-round metric table).  The data-parallel path does
    not compute that column: there ``train_history`` stays empty.

    This half bins and uploads the host arrays; :func:`_fit_device` runs the rounds on what it uploaded."""
    dev = _dev()
    d_bins = torch.from_numpy(np.ascontiguousarray(bins, dtype=np.uint8)).to(dev)
    d_Y = torch.from_numpy(np.ascontiguousarray(Y, dtype=np.float32)).to(dev)
    ev_sets = []
    for name, (ex, ey) in evals.items():
        eb = apply_bins(np.asarray(ex, np.float64), model.cuts)
        db = torch.from_numpy(np.ascontiguousarray(eb, dtype=np.uint8)).to(dev)
        dy = torch.from_numpy(np.ascontiguousarray(np.asarray(ey, np.float32).reshape(len(ex), -1))).to(dev)
        ev_sets.append((name, db, dy))
    return _fit_device(model, d_bins, d_Y, ev_sets, rounds_per_call, dp)


def fit_buffer_bytes(n: int, T: int, F: int, cuts, max_depth: int, nround: int, eval_rows=()) -> int:
    """Device bytes :func:`_fit_device` allocates around ``n`` rows of bins [n, F] and targets [n, T] (both
    included), with an eval set of its own bins and targets per entry of ``eval_rows`` (a set that aliases the
    training rows: count its margin only, as 0 rows plus ``4 * T * n``)."""
    foff = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(c) + 1 for c in cuts])]).astype(np.int32))
    pd = N.query("em_gbdt_partial_doubles", n, T, F, foff.ctypes.data, max_depth)
    if pd < 0:
        raise PlanUnsupported(f"GPU GBDT: no histogram plan for depth {max_depth} x {int(foff[-1])} bins x {T} tasks")
    NN = 2 ** (max_depth + 1) - 1
    rows = n * (F + 4 * T)  # bins + Y
    rows += T * n * (4 + 4 + 4 + 2 + 2)  # margin, g, h, node, node2
    for ne in eval_rows:
        rows += ne * (F + 4 * T) + 4 * T * ne
    trees = nround * T * NN * (1 + 2 + 1 + 4 + 4 + 4)
    return int(rows + 8 * max(pd, 1) + 2 * 8 * T * NN + 8 * 5 * 4096 + trees)


def _fit_device(model, d_bins, d_Y, ev_sets, rounds_per_call: int = 500, dp=None):
    """The rounds, on device tensors: ``d_bins`` uint8 [n, F], ``d_Y`` float32 [n, T] and the eval sets
    ``(name, bins uint8 [ne, F], Y float32 [ne, T])``.  An eval set may alias the training tensors (they are only
    read); every set gets a margin buffer of its own here."""
    dev = d_bins.device
    n, F = d_bins.shape
    T = d_Y.shape[1]
    R, D = model.nround, model.max_depth
    NN = 2 ** (D + 1) - 1
    cells = _Cells(model.cuts, dev)
    margin = torch.empty(T * n, dtype=torch.float32, device=dev)
    stream = N.stream_handle(dev)
    N.call("em_gbdt_init_margin", margin.data_ptr(), T * n, float(model.base_margin), stream)
    ev_names = [name for name, _, _ in ev_sets]
    ev_keep = []
    ev_structs = (_Eval * max(1, len(ev_names)))()
    for i, (name, db, dy) in enumerate(ev_sets):
        ne = db.shape[0]
        em = torch.empty(T * ne, dtype=torch.float32, device=dev)
        N.call("em_gbdt_init_margin", em.data_ptr(), em.numel(), float(model.base_margin), stream)
        ev_keep += [db, dy, em]
        ev_structs[i] = _Eval(db.data_ptr(), dy.data_ptr(), em.data_ptr(), ne)
    g = torch.empty(T * n, dtype=torch.float32, device=dev)
    h = torch.empty_like(g)
    node = torch.empty(T * n, dtype=torch.int16, device=dev)
    node2 = torch.empty_like(node)  # the fused round's double-buffered level nodes
    pdoubles = N.query("em_gbdt_partial_doubles", n, T, F, cells.hp, D)
    if pdoubles < 0:
        raise PlanUnsupported(f"GPU GBDT: no histogram plan for depth {D} x {cells.C} bins x {T} tasks")
    partial = torch.empty(max(pdoubles, 1), dtype=torch.float64, device=dev)
    Gs = torch.zeros(T * NN, dtype=torch.float64, device=dev)
    Hs = torch.zeros_like(Gs)
    mpart = torch.zeros(5 * 4096, dtype=torch.float64, device=dev)  # train + up to 4 eval sets (fused launch)
    status = torch.zeros(R * T * NN, dtype=torch.int8, device=dev)
    feat = torch.zeros(R * T * NN, dtype=torch.int16, device=dev)
    sbin = torch.zeros(R * T * NN, dtype=torch.uint8, device=dev)
    leaf = torch.zeros(R * T * NN, dtype=torch.float32, device=dev)
    gain = torch.zeros_like(leaf)
    cover = torch.zeros_like(leaf)
    hist = torch.zeros(R * (1 + len(ev_names)), dtype=torch.float32, device=dev)
    history = []
    model.train_history = []
    if dp is not None:
        _fit_dp_rounds(model, dp, d_bins, d_Y, n, F, cells, T, margin, ev_names, ev_keep, g, h, node, partial, Gs, Hs,
                       mpart, status, feat, sbin, leaf, gain, cover, history, stream)
    r0 = R if dp is not None else 0
    qbits = quant_bits(model.objective, n, model.hist_mode, dp is not None)
    model.quant_bits_used = qbits
    while r0 < R:
        r1 = min(R, r0 + rounds_per_call)
        N.call("em_gbdt_fit", d_bins.data_ptr(), d_Y.data_ptr(), n, F, cells.hp, cells.dev.data_ptr(), T,
               margin.data_ptr(), ev_structs,
               len(ev_names), r0, r1, D, OBJ[model.objective], MET[model.eval_metric], model.eta, model.lam,
               model.gamma, model.mcw, model.subsample, model.seed & 0xFFFFFFFF, g.data_ptr(), h.data_ptr(),
               node.data_ptr(), node2.data_ptr(), partial.data_ptr(), partial.numel(), Gs.data_ptr(), Hs.data_ptr(), mpart.data_ptr(),
               status.data_ptr(), feat.data_ptr(), sbin.data_ptr(), leaf.data_ptr(), gain.data_ptr(),
               cover.data_ptr(), hist.data_ptr(), qbits,
               # launch flag (csrc/gbdt.hip, the only switch of the round form): 1 = the separate launches instead
               # of the fused round (bit-identity tests); any other bit is an argument error
               1 if getattr(model, "separate_launches", False) else 0, stream)
        hh = hist.view(R, 1 + len(ev_names))[r0:r1].cpu().numpy()
        for i, rnd in enumerate(range(r0, r1)):
            rec = {"round": rnd}
            # XGBoost4J watch order: evals only (train appears if the caller passed it as a watch)
            for j, name in enumerate(ev_names):
                rec[name] = float(hh[i, 1 + j])
            history.append(rec)
            model.train_history.append(float(hh[i, 0]))
            model._log_round(rec)
        r0 = r1
    # the host copy of the ensemble: dtypes converted on the device, one packed device-to-host copy,
    # numpy views of it (per-array host conversions of ~0.5 M nodes cost several ms)
    # (widest dtypes first: every view starts aligned)
    parts = [leaf.to(torch.float64), gain.to(torch.float64), cover.to(torch.float64), feat.to(torch.int32),
             sbin.to(torch.int32), status]
    host = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu().numpy()
    arrs, o = [], 0
    for t, dt in zip(parts, (np.float64, np.float64, np.float64, np.int32, np.int32, np.int8)):
        nb = t.numel() * t.element_size()
        arrs.append(host[o:o + nb].view(dt).reshape(R * T, NN))
        o += nb
    lf, gn, cv, fe, sb, st = arrs
    trees = TreeArrays.from_arrays(D, st, fe, sb, lf, gn, cv)
    model._device_trees = (status, feat, sbin, leaf)
    model._device_cover = cover  # beside them for the explanations (predict_contribs)
    return trees, history


def _fit_dp_rounds(model, dp, d_bins, d_Y, n, F, cells, T, margin, ev_names, ev_keep, g, h, node, partial, Gs, Hs,
                   mpart, status, feat, sbin, leaf, gain, cover, history, stream):
    """C4: per-level histogram all-reduce between the HIP hist and split kernels (stream-ordered,
    no host sync inside a round); metric sums are all-reduced and read back once at the end."""
    import torch.distributed as dist

    R, D = model.nround, model.max_depth
    NN = 2 ** (D + 1) - 1
    dev = d_bins.device
    seed = (model.seed + 0x9E3779B9 * dp.rank) & 0xFFFFFFFF
    msum = torch.zeros(R, max(1, len(ev_names)), 2, dtype=torch.float64, device=dev)
    S = ctypes.c_int64(0)
    obj, met = OBJ[model.objective], MET[model.eval_metric]

    def off(t, k):  # pointer to round-k slice of a [R*T*NN] buffer
        return t.data_ptr() + k * T * NN * t.element_size()

    for rnd in range(R):
        N.call("em_gbdt_dp_round_begin", rnd, T, n, D, margin.data_ptr(), d_Y.data_ptr(), g.data_ptr(), h.data_ptr(),
               node.data_ptr(), obj, model.subsample, seed, off(status, rnd), off(feat, rnd), off(sbin, rnd),
               off(gain, rnd), stream)
        for level in range(D):
            N.call("em_gbdt_dp_level_hist", level, d_bins.data_ptr(), g.data_ptr(), h.data_ptr(), node.data_ptr(), T, n,
                   F, cells.hp, cells.dev.data_ptr(), partial.data_ptr(), partial.numel(), ctypes.byref(S), stream)
            dist.all_reduce(partial[:S.value], group=dp.group)
            N.call("em_gbdt_dp_level_split", level, d_bins.data_ptr(), partial.data_ptr(), T, n, F,
                   cells.dev.data_ptr(), cells.C, D,
                   node.data_ptr(), Gs.data_ptr(), Hs.data_ptr(), off(status, rnd), off(feat, rnd), off(sbin, rnd),
                   off(gain, rnd), model.lam, model.mcw, stream)
        N.call("em_gbdt_dp_round_end", T, n, D, margin.data_ptr(), node.data_ptr(), off(status, rnd), off(feat, rnd),
               off(gain, rnd), Gs.data_ptr(), Hs.data_ptr(), off(leaf, rnd), off(cover, rnd), model.lam, model.gamma,
               model.eta, stream)
        for j, name in enumerate(ev_names):
            db, dy, em = ev_keep[3 * j:3 * j + 3]
            ne = db.shape[0]
            N.call("em_gbdt_predict", db.data_ptr(), em.data_ptr(), T, ne, F, D, rnd * T, rnd * T + T,
                   status.data_ptr(), feat.data_ptr(), sbin.data_ptr(), leaf.data_ptr(), stream)
            N.call("em_gbdt_metric_sum", em.data_ptr(), dy.data_ptr(), T, ne, obj, met, mpart.data_ptr(),
                   msum[rnd, j, :1].data_ptr(), stream)
            msum[rnd, j, 1] = float(ne if met >= 3 else T * ne)
    if ev_names:
        dist.all_reduce(msum, group=dp.group)
    ms = msum.cpu().numpy()
    for rnd in range(R):
        rec = {"round": rnd}
        for j, name in enumerate(ev_names):
            v = ms[rnd, j, 0] / max(ms[rnd, j, 1], 1.0)
            rec[name] = float(np.sqrt(v)) if model.eval_metric == "rmse" else float(v)
        history.append(rec)
        model._log_round(rec)


def _device_margin(model, d_bins: torch.Tensor) -> torch.Tensor:
    """em_gbdt_predict on device bins uint8 [n, F]: the margins as float32 [T, n] on the device."""
    dev, tr = d_bins.device, model.trees
    n, F = d_bins.shape
    T = model.n_tasks
    dt = getattr(model, "_device_trees", None)
    if dt is None:
        dt = (torch.from_numpy(tr.status.reshape(-1)).to(dev), torch.from_numpy(tr.feat.astype(np.int16).reshape(-1)).to(dev),
              torch.from_numpy(tr.sbin.astype(np.uint8).reshape(-1)).to(dev),
              torch.from_numpy(tr.leaf.astype(np.float32).reshape(-1)).to(dev))
        model._device_trees = dt
    status, feat, sbin, leaf = dt
    margin = torch.full((T * n,), float(model.base_margin), dtype=torch.float32, device=dev)
    N.call("em_gbdt_predict", d_bins.data_ptr(), margin.data_ptr(), T, n, F, tr.max_depth, 0, tr.n_trees,
           status.data_ptr(), feat.data_ptr(), sbin.data_ptr(), leaf.data_ptr(), N.stream_handle(dev))
    return margin.view(T, n)


def predict_margin(model, X):
    bins = apply_bins(X, model.cuts)
    d_bins = torch.from_numpy(np.ascontiguousarray(bins, dtype=np.uint8)).to(_dev())
    return _device_margin(model, d_bins).t().cpu().numpy().astype(np.float64)


def predict_margin_rows(model, d_bins: torch.Tensor) -> torch.Tensor:
    """Margins of device bins uint8 [n, F] as float32 [n, 64] on the device, task ``t`` in column ``t`` and zeros
    from column T on: the logit rows ``draw_metrics`` / ``draw_tickets`` read (T <= 64)."""
    out = torch.zeros(d_bins.shape[0], 64, dtype=torch.float32, device=d_bins.device)
    out[:, :model.n_tasks] = _device_margin(model, d_bins).t()
    return out


# ----------------------------------------------------------------------------- explanations (csrc/gbdt_shap.hip)
SHAP_CHUNK_BYTES = 256 << 20  # default chunk_rows: at most this much contribution output per launch


def _explain_trees(model, sbin_host):
    """(status, feat, sbin, leaf, cover) on the device: what ``fit`` left there, or copies of the host trees
    (a loaded checkpoint, a numpy fit) with the given ``sbin``."""
    dt, cv = getattr(model, "_device_trees", None), getattr(model, "_device_cover", None)
    if dt is not None and cv is not None and model.cuts is not None:
        return (*dt, cv)
    cached = getattr(model, "_explain_device", None)
    if cached is not None and cached[0] is model.trees:
        return cached[1]
    dev, tr = _dev(), model.trees
    arrs = (torch.from_numpy(np.ascontiguousarray(tr.status, dtype=np.int8).reshape(-1)).to(dev),
            torch.from_numpy(tr.feat.astype(np.int16).reshape(-1)).to(dev),
            torch.from_numpy(np.asarray(sbin_host).astype(np.uint8).reshape(-1)).to(dev),
            torch.from_numpy(tr.leaf.astype(np.float32).reshape(-1)).to(dev),
            torch.from_numpy(tr.cover.astype(np.float32).reshape(-1)).to(dev))
    model._explain_device = (tr, arrs)
    return arrs


def _explain_plan(model, need_lds: bool):
    """Validate the trees on the host (the kernels index ``bins`` by ``feat``) and check the plan; returns
    (cuts, device trees, F)."""
    from . import gbdt_explain as E

    tr = model.trees
    F = E.num_features(model)
    E.validate_trees(tr, F)
    cuts, sbin_host = E.model_bins(model)
    if any(len(c) > 255 for c in cuts):
        raise PlanUnsupported("GPU GBDT supports at most 256 bins per feature")
    if F > 32767:
        raise PlanUnsupported("GPU GBDT explanations index features with 16 bits")
    if need_lds and N.query("em_gbdt_shap_lds_bytes", F, tr.max_depth) < 0:
        raise PlanUnsupported(f"GPU TreeSHAP: no plan for max_depth {tr.max_depth} with {F} features (the plan covers "
                              f"max_depth <= 8 and a row tile, 324 bytes per feature, within 160 KB of LDS)")
    if not need_lds and not 1 <= tr.max_depth <= 12:
        raise PlanUnsupported(f"GPU leaf index: max_depth {tr.max_depth} outside [1, 12]")
    return cuts, _explain_trees(model, sbin_host), F


def _bins_for(model, X, cuts, F):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != F:
        raise ValueError(f"X must be [n, {F}], got {X.shape}")
    return np.ascontiguousarray(apply_bins(X, cuts), dtype=np.uint8)


def _shap_tables(model, dtrees, F):
    """The device path table of every tree (em_gbdt_shap_paths), built once per set of device trees."""
    cached = getattr(model, "_shap_paths", None)
    if cached is not None and cached[0] is dtrees[0]:
        return cached[1]
    dev = dtrees[0].device
    tr = model.trees
    K, D = tr.n_trees, tr.max_depth
    E_ = K * (2 ** (D + 1) - 1)
    pd = torch.empty(E_, dtype=torch.int32, device=dev)
    pleaf = torch.empty(E_, dtype=torch.float32, device=dev)
    pf, plo, phi = (torch.empty(E_ * D, dtype=torch.int32, device=dev) for _ in range(3))
    pz = torch.empty(E_ * D, dtype=torch.float32, device=dev)
    pbias = torch.empty(E_, dtype=torch.float64, device=dev)
    status, feat, sbin, leaf, cover = dtrees
    N.call("em_gbdt_shap_paths", K, D, F, status.data_ptr(), feat.data_ptr(), sbin.data_ptr(), leaf.data_ptr(),
           cover.data_ptr(), pd.data_ptr(), pleaf.data_ptr(), pf.data_ptr(), plo.data_ptr(), phi.data_ptr(), pz.data_ptr(),
           pbias.data_ptr(), N.stream_handle(dev))
    tables = (pd, pleaf, pf, plo, phi, pz, pbias)
    model._shap_paths = (dtrees[0], tables)
    return tables


def predict_contribs(model, X, iteration_range=None, chunk_rows=None):
    """float32 [n, T, F+1] (GBDT.predict_contribs).  Rows go through the kernel ``chunk_rows`` at a time, so the
    [T, chunk, F+1] device output is bounded; a row's result depends on the row only."""
    from . import gbdt_explain as E

    cuts, dtrees, F = _explain_plan(model, need_lds=True)
    bins = _bins_for(model, X, cuts, F)
    k0, k1 = E._tree_range(model, iteration_range)
    n, T, tr = bins.shape[0], model.n_tasks, model.trees
    out = np.empty((n, T, F + 1), dtype=np.float32)
    if n == 0:
        return out
    if chunk_rows is None:
        chunk_rows = max(256, SHAP_CHUNK_BYTES // (T * (F + 1) * 4) // 256 * 256)
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be positive")
    chunk_rows = min(chunk_rows, ((1 << 31) - 1) // F)
    dev = dtrees[0].device
    tables = _shap_tables(model, dtrees, F)
    bias = torch.empty(T, dtype=torch.float32, device=dev)
    stream = N.stream_handle(dev)
    for a in range(0, n, chunk_rows):
        b = min(n, a + chunk_rows)
        d_bins = torch.from_numpy(bins[a:b]).to(dev)
        d_out = torch.empty((T, b - a, F + 1), dtype=torch.float32, device=dev)
        N.call("em_gbdt_shap", d_bins.data_ptr(), b - a, F, T, tr.max_depth, tr.n_trees, k0, k1, float(model.base_margin),
               *(t.data_ptr() for t in tables), bias.data_ptr(), d_out.data_ptr(), stream)
        out[a:b] = d_out.permute(1, 0, 2).cpu().numpy()
    return out


def predict_leaf(model, X):
    """int32 [n, n_trees] heap indices (GBDT.predict_leaf)."""
    cuts, dtrees, F = _explain_plan(model, need_lds=False)
    bins = _bins_for(model, X, cuts, F)
    n, tr = bins.shape[0], model.trees
    if n == 0 or tr.n_trees == 0:
        return np.zeros((n, tr.n_trees), dtype=np.int32)
    dev = dtrees[0].device
    status, feat, sbin = dtrees[:3]
    rows = max(1, SHAP_CHUNK_BYTES // (4 * tr.n_trees))
    out = np.empty((n, tr.n_trees), dtype=np.int32)
    for a in range(0, n, rows):
        b = min(n, a + rows)
        d_bins = torch.from_numpy(bins[a:b]).to(dev)
        d_out = torch.empty((b - a, tr.n_trees), dtype=torch.int32, device=dev)
        N.call("em_gbdt_leaf_index", d_bins.data_ptr(), d_out.data_ptr(), b - a, F, tr.max_depth, tr.n_trees,
               status.data_ptr(), feat.data_ptr(), sbin.data_ptr(), N.stream_handle(dev))
        out[a:b] = d_out.cpu().numpy()
    return out
