"""Python face of ``csrc/draw_counts.hip``: the transition-count baseline on device draw masks.

:func:`pair_counts` counts, over a window of the masks, how often bit ``a`` of a draw and bit ``b`` of the draw
``lag`` steps later are both set (integers, exact); :func:`count_logits` scores samples with the table that
``models.count_table.weights_from_counts`` makes of those counts, bit for bit as ``count_table.logits_np``.  The
masks are the 8-byte feature masks every draw kernel reads (``ops.fused_mlp.rows_to_masks``,
``data.device_gen.generate_masks``).  Every argument error is a ``ValueError`` raised before anything is launched
or written."""
from __future__ import annotations

import torch

from . import _native as N
from .fused_mlp import _check_draws
from .tree_inputs import _check_masks, _check_out, _check_window

N.register_signatures({
    "em_pair_counts": (N._i32, [N._c_void_p, N._i64, N._i64, N._i64, N._i32, N._c_void_p, N._c_void_p]),
    "em_count_logits": (N._i32, [N._c_void_p, N._i64, N._c_void_p, N._i64, N._i64, N._i32, N._c_void_p, N._c_void_p,
                                 N._c_void_p, N._i64, N._c_void_p]),
})

MAX_LAG = 4  # the kernels' lag / lags range, as ops.tree_inputs.MAX_LAGS
MAX_COUNT = 1 << 40  # samples per pair_counts launch (its 32-bit block counters cannot wrap below that)


def pair_counts(masks: torch.Tensor, lag: int, first: int = 0, count: int | None = None,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """int64 [64, 64] on the device: ``C[a, b]`` = number of ``t`` in ``[first, first + count)`` with bit ``a`` of
    ``masks[t]`` and bit ``b`` of ``masks[t + lag]`` set; rows and columns 62-63 are 0.  ``lag`` in 0..4
    (0: same-draw co-occurrence, the diagonal is the bit counts).  ``count=None``: every ``t`` from ``first`` on.
    ``out``: the tensor to fill."""
    n = _check_masks(masks)
    lag, first = int(lag), int(first)
    if not 0 <= lag <= MAX_LAG:
        raise ValueError(f"pair_counts: lag must be in 0..{MAX_LAG}, got {lag}")
    count = n - lag - first if count is None else int(count)
    _check_window(n, first, count, lag, "pair_counts")
    if count > MAX_COUNT:
        raise ValueError(f"pair_counts: at most 2^40 samples per call (got {count}); add the counts of several windows")
    if out is None:
        out = torch.empty(64, 64, dtype=torch.int64, device=masks.device)
    else:
        _check_out(out, "out", torch.int64, (64, 64), masks.device)
    N.call("em_pair_counts", masks.data_ptr(), n, first, count, lag, out.data_ptr(), N.stream_handle(masks.device))
    return out


def _check_table(table: torch.Tensor, prior: torch.Tensor, device) -> int:
    N.check_cuda(table, "table", torch.float32)
    N.check_cuda(prior, "prior", torch.float32)
    if table.dim() != 3 or tuple(table.shape[1:]) != (64, 64) or not 1 <= table.shape[0] <= MAX_LAG:
        raise ValueError(f"table must be float32 [lags, 64, 64] with lags in 1..{MAX_LAG}")
    if tuple(prior.shape) != (64,):
        raise ValueError("prior must be float32 [64]")
    if table.device != device or prior.device != device:
        raise ValueError(f"table and prior must be on {device}")
    return table.shape[0]


def count_logits(masks: torch.Tensor, B: int, table: torch.Tensor, prior: torch.Tensor, offset: int = 0,
                 sidx: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """float32 [B, 64] on the device: row ``s`` scores sample ``i = sidx[s]`` (or ``offset + s``), which reads the
    draws ``i .. i + lags - 1`` and whose target is draw ``i + lags`` (it must exist).  ``lags`` is ``table.shape[0]``.
    ``out``: [>= B, >= 64] float32 rows to fill, with a row stride that is a multiple of 4 floats (columns 0..63 of
    each row are written)."""
    if not isinstance(masks, torch.Tensor):
        raise ValueError("masks must be a GPU tensor")
    B, offset = int(B), int(offset)
    N.check_cuda(masks, "masks", torch.int64)
    lags = _check_table(table, prior, masks.device)
    if B < 1:
        raise ValueError(f"count_logits: needs at least one sample (got {B})")
    if masks.dim() != 1 or masks.shape[0] <= lags:
        raise ValueError(f"count_logits: lags={lags} needs more than {lags} masks")
    _check_draws(masks[lags - 1:], sidx, B, offset)
    if out is None:
        out = torch.empty(B, 64, dtype=torch.float32, device=masks.device)
    else:
        N.check_cuda(out, "out", torch.float32, contiguous=False)
        if (out.dim() != 2 or out.shape[0] < B or out.shape[1] < 64 or out.stride(1) != 1 or out.stride(0) % 4
                or out.stride(0) < 64 or out.data_ptr() % 16 or out.device != masks.device):
            raise ValueError("out must be [>= B, >= 64] float32 rows on the masks' device, 16-byte aligned, with a row "
                             "stride that is a multiple of 4")
    N.call("em_count_logits", masks.data_ptr(), masks.shape[0], N.ptr(sidx), B, offset, lags, table.data_ptr(),
           prior.data_ptr(), out.data_ptr(), out.stride(0), N.stream_handle(masks.device))
    return out
