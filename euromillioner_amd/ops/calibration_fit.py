"""Python face of ``csrc/calibration_fit.hip``: scaling statistics of device logits, the Newton fit over them and
the apply pass.

The specification is :mod:`euromillioner_amd.scaling` (numpy).  The fit is ``scaling.fit`` itself: the engines differ
only in who computes the statistics, and here that is one kernel pass over logits that never leave the device."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import scaling as SC
from . import _native as N
from .fused_mlp import LOSS_KINDS, _check_draws

N.register_signatures({
    "em_scaling_blocks": (ctypes.c_int, [ctypes.c_int64]),
    "em_scaling_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    "em_scaling_apply": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
})


def scaling_blocks(B: int) -> int:
    """Rows of the partials that :func:`scaling_stats` returns (one per 256-row block)."""
    return int(N.query("em_scaling_blocks", int(B)))


def _check_rows(t: torch.Tensor, name: str, B: int) -> None:
    N.check_cuda(t, name, torch.float32, contiguous=False)
    if (t.dim() != 2 or t.shape[1] < 64 or t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < 64
            or t.shape[0] < B):
        raise ValueError(f"{name} must be [>= B, >= 64] fp32 rows with a row stride that is a multiple of 4")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")


def _check_args(logits, masks, B, loss, a, b, offset, sidx) -> tuple[np.ndarray, np.ndarray]:
    """Every refusal of :func:`scaling_stats`, as a ``ValueError`` before anything is allocated or launched.
    Returns the float32 ``(a, b)``."""
    a32, b32 = SC.check_ab(a, b, loss)  # (unknown loss, bad scales or shifts)
    B = int(B)
    if B < 1:
        raise ValueError("B must be at least 1")
    _check_rows(logits, "logits", B)
    _check_draws(masks, sidx, B, offset)
    if masks.device != logits.device or (sidx is not None and sidx.device != logits.device):
        raise ValueError("logits, masks and sample_idx must be on one device")
    return a32, b32


def _host_pair(v: np.ndarray):
    buf = (ctypes.c_float * 2)(float(v[0]), float(v[1]))
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def scaling_stats(logits: torch.Tensor, masks: torch.Tensor, B: int, loss: str, a=(1.0, 1.0), b=(0.0, 0.0),
                  offset: int = 0, sidx: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Statistics partials of the first B rows of ``logits`` [>= B, >= 64] (fp32, row stride a multiple of 4) at
    ``(a, b)``, row s scored against ``masks[idx + 1]`` with ``idx = sidx[s]`` or ``offset + s``: a device tensor fp32
    [blocks, 2, 6] (``scaling.STATS``), one row per 256-row block.  Sum it with :func:`sum_scaling`.  ``out``: the
    tensor to fill."""
    a32, b32 = _check_args(logits, masks, B, loss, a, b, offset, sidx)
    B = int(B)
    shape = (scaling_blocks(B), 2, 6)
    if out is not None:
        N.check_cuda(out, "out", torch.float32)
        if tuple(out.shape) != shape or out.device != logits.device:
            raise ValueError(f"out must be fp32 {list(shape)} on {logits.device}")
    else:
        out = torch.empty(shape, dtype=torch.float32, device=logits.device)
    (abuf, ap), (bbuf, bp) = _host_pair(a32), _host_pair(b32)
    N.call("em_scaling_stats", logits.data_ptr(), logits.stride(0), masks.data_ptr(), N.ptr(sidx), B, int(offset),
           LOSS_KINDS[loss], ap, bp, out.data_ptr(), N.stream_handle(logits.device))
    return out


def sum_scaling(parts: torch.Tensor) -> np.ndarray:
    """Partials -> the host totals ``scaling.stats_np`` returns: float64 [2, 6]."""
    return parts.double().sum(0).cpu().numpy()


def apply_scaling(logits: torch.Tensor, B: int, a, b, out: torch.Tensor | None = None) -> torch.Tensor:
    """``out[s, o] = fl32(fl32(a[g] z) + b[g])`` for the first B rows and o < 62, 0 in columns 62-63 (bit-equal to
    ``scaling.apply_np``).  ``out``: fp32 [>= B, >= 64] rows to fill, which may be ``logits`` itself; by default a
    new [B, 64] tensor.  Returns ``out``."""
    a32, b32 = SC.check_ab(a, b, "bce")
    B = int(B)
    if B < 1:
        raise ValueError("B must be at least 1")
    _check_rows(logits, "logits", B)
    if out is not None:
        _check_rows(out, "out", B)
        if out.device != logits.device:
            raise ValueError("logits and out must be on one device")
        if out.data_ptr() == logits.data_ptr() and out.stride(0) != logits.stride(0):
            raise ValueError("in place, out must have the row stride of logits")
    else:
        out = torch.empty(B, 64, dtype=torch.float32, device=logits.device)
    (abuf, ap), (bbuf, bp) = _host_pair(a32), _host_pair(b32)
    N.call("em_scaling_apply", logits.data_ptr(), logits.stride(0), B, ap, bp, out.data_ptr(), out.stride(0),
           N.stream_handle(logits.device))
    return out


def fit_device(logits: torch.Tensor, target_masks: torch.Tensor, B: int, loss: str, offset: int = 0,
               sidx: torch.Tensor | None = None) -> dict:
    """``scaling.fit`` over :func:`scaling_stats`: every Newton pass is one kernel launch over the B device rows and
    a [blocks, 2, 6] read-back.  Returns what ``scaling.fit`` returns."""
    _check_args(logits, target_masks, B, loss, (1.0, 1.0), (0.0, 0.0), offset, sidx)
    parts = torch.empty(scaling_blocks(int(B)), 2, 6, dtype=torch.float32, device=logits.device)

    def stats(a, b):
        return sum_scaling(scaling_stats(logits, target_masks, B, loss, a, b, offset=offset, sidx=sidx, out=parts))

    return SC.fit(stats, loss)
