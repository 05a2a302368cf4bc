"""Python face of ``csrc/calibration.hip``: calibration totals of device logits (reliability table, Brier sum).

The specification is :mod:`euromillioner_amd.calibration` (numpy); the kernel consumes the logits that a model's
``logits()`` already produced, next to ``draw_metrics`` on the same rows, so they never leave the device."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import calibration as CAL
from . import _native as N
from .fused_mlp import LOSS_KINDS, METRIC_NAMES, _check_draws, draw_metrics

N.register_signatures({
    "em_calibration_blocks": (ctypes.c_int, [ctypes.c_int64]),
    "em_draw_calibration": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]),
})


def calibration_blocks(B: int) -> int:
    """Rows of the partials that :func:`draw_calibration` returns (one per 256-row block)."""
    return int(N.query("em_calibration_blocks", int(B)))


def _check_args(logits, masks, B, loss, edges, offset, sidx) -> np.ndarray:
    """Every refusal of :func:`draw_calibration`, as a ``ValueError`` before anything is allocated or launched.
    Returns the float32 x-space edge table."""
    ex = CAL.edges_x(edges, loss)  # (unknown loss, bad edges)
    B = int(B)
    if B < 1:
        raise ValueError("B must be at least 1")
    N.check_cuda(logits, "logits", torch.float32, contiguous=False)
    if (logits.dim() != 2 or logits.shape[1] < 64 or logits.stride(1) != 1 or logits.stride(0) % 4
            or logits.stride(0) < 64 or logits.shape[0] < B):
        raise ValueError("logits must be [>= B, >= 64] fp32 rows with a row stride that is a multiple of 4")
    if logits.data_ptr() % 16:
        raise ValueError("logits must be 16-byte aligned")
    _check_draws(masks, sidx, B, offset)
    if masks.device != logits.device or (sidx is not None and sidx.device != logits.device):
        raise ValueError("logits, masks and sample_idx must be on one device")
    return ex


def draw_calibration(logits: torch.Tensor, masks: torch.Tensor, B: int, loss: str, edges=CAL.DEFAULT_EDGES,
                     offset: int = 0, sidx: torch.Tensor | None = None, want_bins: bool = False,
                     out: dict | None = None) -> dict:
    """Calibration partials of the first B rows of ``logits`` [>= B, >= 64] (fp32, row stride a multiple of 4), row s
    scored against ``masks[idx + 1]`` with ``idx = sidx[s]`` or ``offset + s`` (as ``draw_metrics``).

    Returns device tensors, one row per 256-row block: ``counts`` and ``hits`` int32 [blocks, 2, 16], ``sum_q`` fp32
    [blocks, 2, 16], ``brier`` fp32 [blocks, 2] and, with ``want_bins``, ``bins`` uint8 [B, 64] (the bin of every
    element, pads 0).  Sum them with :func:`sum_calibration`.  ``out``: tensors of those names to fill."""
    ex = _check_args(logits, masks, B, loss, edges, offset, sidx)
    B, dev = int(B), logits.device
    nb = calibration_blocks(B)
    shapes = {"counts": ((nb, 2, 16), torch.int32), "hits": ((nb, 2, 16), torch.int32),
              "sum_q": ((nb, 2, 16), torch.float32), "brier": ((nb, 2), torch.float32)}
    if want_bins:
        shapes["bins"] = ((B, 64), torch.uint8)
    res = {}
    for name, (shape, dtype) in shapes.items():
        if out is not None and name in out:
            t = out[name]
            N.check_cuda(t, name, dtype)
            if tuple(t.shape) != shape or t.device != dev:
                raise ValueError(f"out[{name!r}] must be {dtype} {list(shape)} on {dev}")
        else:
            t = torch.empty(shape, dtype=dtype, device=dev)
        res[name] = t
    ebuf = (ctypes.c_float * max(len(ex), 1))(*[float(v) for v in ex])
    N.call("em_draw_calibration", logits.data_ptr(), logits.stride(0), masks.data_ptr(), N.ptr(sidx), B, int(offset),
           LOSS_KINDS[loss], ctypes.cast(ebuf, ctypes.c_void_p), len(ex), res["counts"].data_ptr(),
           res["hits"].data_ptr(), res["sum_q"].data_ptr(), res["brier"].data_ptr(), N.ptr(res.get("bins")),
           N.stream_handle(dev))
    return res


def sum_calibration(parts: dict) -> dict:
    """Partials -> host totals in the shape ``calibration_np`` returns: ``counts`` / ``hits`` int64 [2, 16], ``sum_q``
    float64 [2, 16], ``brier`` float64 [2]."""
    return {"counts": parts["counts"].to(torch.int64).sum(0).cpu().numpy(),
            "hits": parts["hits"].to(torch.int64).sum(0).cpu().numpy(),
            "sum_q": parts["sum_q"].double().sum(0).cpu().numpy(),
            "brier": parts["brier"].double().sum(0).cpu().numpy()}


def calibrate_model(model, masks: torch.Tensor, B: int, loss: str, edges=CAL.DEFAULT_EDGES, offset: int = 0,
                    sidx: torch.Tensor | None = None, chunk: int = 1 << 20,
                    target_masks: torch.Tensor | None = None) -> dict:
    """Score B samples of a model: per chunk ``model.logits`` once, then ``draw_metrics`` and :func:`draw_calibration`
    on those logits (the logits of one chunk are the only intermediate).  ``target_masks``: the masks as the scoring
    sees them when the model's target is not ``masks[i + 1]`` (lag windows).  Returns ``{"val": the METRIC_NAMES dict
    of ``model.evaluate``, "calibration": calibration.report(...)}``; the integers do not depend on ``chunk``."""
    if getattr(model, "group", None) is not None:
        raise ValueError("calibrate_model is single-process (no process group)")
    edges = CAL.check_edges(edges)
    CAL.check_loss(loss)
    B = int(B)
    if B < 1:
        raise ValueError("B must be at least 1")
    if chunk < 1:
        raise ValueError("chunk >= 1")
    tm = masks if target_masks is None else target_masks
    _check_draws(tm, sidx, B, offset)
    return calibrate_logits(lambda b, o, si: model.logits(masks, b, offset=o, sidx=si), tm, B, loss, edges,
                            offset=offset, sidx=sidx, chunk=chunk)


def calibrate_logits(logits_of, target_masks: torch.Tensor, B: int, loss: str, edges=CAL.DEFAULT_EDGES,
                     offset: int = 0, sidx: torch.Tensor | None = None, chunk: int = 1 << 20) -> dict:
    """The loop of :func:`calibrate_model` over any source of device logits: ``logits_of(b, offset, sidx)`` returns
    the fp32 [b, >= 64] logits of the chunk's samples, which are scored against ``target_masks[idx + 1]``."""
    tot8 = np.zeros(8, dtype=np.float64)
    totals = None
    done = 0
    while done < B:
        b = min(chunk, B - done)
        o = offset + done if sidx is None else 0
        si = None if sidx is None else sidx[done:done + b]
        lg = logits_of(b, o, si)
        tot8 += draw_metrics(lg, target_masks, b, loss=loss, offset=o, sidx=si).double().sum(0).cpu().numpy()
        totals = CAL.add_totals(totals, sum_calibration(draw_calibration(lg, target_masks, b, loss, edges, offset=o,
                                                                         sidx=si)))
        done += b
    cnt = max(tot8[7], 1.0)
    val = {k: float(tot8[i] / cnt) for i, k in enumerate(METRIC_NAMES[:-1])}
    val["count"] = int(tot8[7])
    return {"val": val, "calibration": CAL.report(totals, B, loss, edges)}
