"""fp64 reference of the calibration totals (tests/test_calibration_cpu.py, tests/test_calibration_gpu.py), written
from the definitions with plain loops over the 62 outputs and the edges; independent of
euromillioner_amd.calibration.  Nothing here touches the GPU.

The one thing shared with the engines is the float32 x-space edge table (``ex``): the caller passes it in.

Per element the reference gives the fp64 ``x``, the bin ``number of edges e with x >= e`` (x in fp64 against the
float32 edge widened to fp64) and ``near``: ``|x - e| < _fused_ref.THR_MARGIN`` for some edge, the project's own 1e-3
margin for the kernels' fast exp / log.  Under bce x is the fp32 logit itself, so the fp64 comparison is the fp32
comparison and an engine must reproduce the bins exactly, near or not; under softmax an engine that forms x in fp32
may put a ``near`` element one bin across that edge.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import _fused_ref as R

K_NOMINAL = (5.0, 2.0)
NEAR_CAP = 0.05  # largest share of near elements per family under softmax (the slack of the GPU test)
GROUP_COLS = (range(0, 50), range(50, 62))


def reference(z, Y, loss: str, ex) -> dict:
    """z [B, >= 62] logits, Y [B, 62] 0 / 1 targets, ex: float32 x-space edges (ascending).  Returns per element
    ``x``, ``q`` (fp64 [B, 62]), ``bins`` (int64 [B, 62]), ``near`` (bool [B, 62]) and the totals ``counts``, ``hits``
    (int64 [2, 16]), ``sum_q`` (fp64 [2, 16]), ``brier`` (fp64 [2])."""
    z = np.asarray(z, dtype=np.float64)[:, :62]
    y = np.asarray(Y, dtype=np.float64)[:, :62]
    ex = [float(e) for e in np.asarray(ex, dtype=np.float32)]
    B = z.shape[0]
    x, q, t = np.zeros((B, 62)), np.zeros((B, 62)), np.zeros((B, 62))
    for g, cols in enumerate(GROUP_COLS):
        if loss == "softmax":
            top = np.full(B, -np.inf)
            for o in cols:
                top = np.maximum(top, z[:, o])
            tot = np.zeros(B)
            for o in cols:
                tot += np.exp(z[:, o] - top)
            lse = top + np.log(tot)
            for o in cols:
                x[:, o] = z[:, o] - lse
                q[:, o] = np.exp(x[:, o])
                t[:, o] = y[:, o] / K_NOMINAL[g]
        elif loss == "bce":
            for o in cols:
                x[:, o] = z[:, o]
                with np.errstate(over="ignore"):
                    q[:, o] = 1.0 / (1.0 + np.exp(-z[:, o]))
                t[:, o] = y[:, o]
        else:
            raise ValueError(loss)
    bins = np.zeros((B, 62), dtype=np.int64)
    near = np.zeros((B, 62), dtype=bool)
    for e in ex:
        bins += x >= e
        near |= np.abs(x - e) < R.THR_MARGIN
    out = {"x": x, "q": q, "bins": bins, "near": near, "y": y.astype(np.int64)}
    out.update(totals_from_bins(bins, y, q, t))
    return out


def totals_from_bins(bins, y, q=None, t=None) -> dict:
    """counts / hits (and sum_q / brier when q, t are given) of per-element bins [B, 62] and targets y [B, 62]."""
    bins, y = np.asarray(bins).astype(np.int64)[:, :62], np.asarray(y).astype(np.int64)[:, :62]
    out = {"counts": np.zeros((2, 16), dtype=np.int64), "hits": np.zeros((2, 16), dtype=np.int64)}
    if q is not None:
        out["sum_q"], out["brier"] = np.zeros((2, 16)), np.zeros(2)
    for g, cols in enumerate(GROUP_COLS):
        for o in cols:
            for b in range(16):
                sel = bins[:, o] == b
                out["counts"][g, b] += int(sel.sum())
                out["hits"][g, b] += int(y[sel, o].sum())
                if q is not None:
                    out["sum_q"][g, b] += float(q[sel, o].sum())
            if q is not None:
                out["brier"][g] += float(((q[:, o] - t[:, o]) ** 2).sum())
    return out


def edges_x_ref(edges, loss: str) -> list[float]:
    """The x-space edges from math.log, in fp64 (the engines' float32 table must be their rounding)."""
    return [math.log(p / (1.0 - p)) if loss == "bce" else math.log(p) for p in edges]


@functools.lru_cache(maxsize=None)
def case(family: str, B: int = 1301, offset: int = 0, sidx_seed: int | None = None):
    """(z fp32 [B, 64] with pads 0, Y [B, 62], target masks int64 [B], sidx or None) of one test case: rows of
    ``R.draw_masks()`` from ``offset`` (or through a sample index with repeats), logits of ``family``."""
    masks = R.draw_masks()
    sidx = None
    if sidx_seed is not None:
        sidx = torch.randint(0, 5000, (B,), generator=torch.Generator().manual_seed(sidx_seed), dtype=torch.int32)
        if B > 262:
            sidx[250:262] = sidx[0]
    _, Y = R.xy(masks, B, offset, sidx=sidx)
    z = R.logit_family(family, Y, seed=B + offset + (77 if sidx is not None else 0))
    idx = sidx.long() if sidx is not None else torch.arange(offset, offset + B)
    return z, Y, masks[idx + 1].numpy().copy(), sidx


@functools.lru_cache(maxsize=None)
def case_reference(family: str, loss: str, ex: tuple, B: int = 1301, offset: int = 0, sidx_seed: int | None = None):
    z, Y, _, _ = case(family, B, offset, sidx_seed)
    return reference(z.numpy(), Y.numpy(), loss, np.asarray(ex, dtype=np.float32))


def check_result(res: dict, loss: str, engine: str, n_edges: int = 15) -> None:
    """Keys and invariants of the JSON result of ``evaluate``."""
    for k in ("model", "checkpoint", "engine", "rows", "val", "calibration", "edges"):
        assert k in res, k
    rows = res["rows"]
    assert res["engine"] == engine and res["loss"] == loss and rows >= 1 and len(res["edges"]) == n_edges
    assert res["val"]["count"] == rows
    for k in ("loss", "acc", "acc_thr", "hits_main", "hits_star", "exact", "trivial_acc"):
        assert math.isfinite(res["val"][k]), k
    for name, width, k in (("main", 50, 5), ("stars", 12, 2)):
        g = res["calibration"][name]
        assert len(g["bins"]) == 16
        assert sum(r["count"] for r in g["bins"]) == g["count"] == width * rows
        assert g["hits"] == k * rows
        assert all(r["count"] == 0 for r in g["bins"][n_edges + 1:])
        assert g["brier"] >= 0 and 0 <= g["ece"] <= 1
        for r in g["bins"]:
            if r["count"]:
                assert 0 <= r["mean_q"] <= 1 and 0 <= r["observed"] <= 1
            else:
                assert r["mean_q"] is None and r["observed"] is None
