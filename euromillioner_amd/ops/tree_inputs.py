"""Python face of ``csrc/tree_inputs.hip``: draw masks -> the tree models' inputs on the device.

The masks are the 8-byte feature masks every draw kernel reads (``ops.fused_mlp.rows_to_masks``,
``data.device_gen.generate_masks``: bit n-1 main number n, bit 49+s star s).  The forest trains on packed
lag-window rows (:func:`rf_rows` == ``data.draws.lag_features`` + ``models.forest.pack_bits``), the GBDT on one
uint8 bin and one float32 target per column (:func:`gbdt_draw_inputs` == ``multi_hot`` + ``apply_bins`` with the
cuts of :func:`cuts_from_bit_counts`).  Every argument error is a ``ValueError`` raised before anything is
launched or written."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as N

N.register_signatures({
    "em_rf_lag_rows": (N._i32, [N._c_void_p, N._i64, N._i64, N._i64, N._i32, N._c_void_p, N._i32, N._c_void_p,
                                N._c_void_p]),
    "em_mask_bit_count_blocks": (N._i32, [N._i64]),
    "em_mask_bit_counts": (N._i32, [N._c_void_p, N._i64, N._i64, N._i64, N._c_void_p, N._c_void_p, N._c_void_p]),
    "em_gbdt_draw_inputs": (N._i32, [N._c_void_p, N._i64, N._i64, N._i64, ctypes.c_uint64, N._c_void_p, N._c_void_p,
                                     N._c_void_p]),
})

NF = 62  # features / targets per draw
MAX_LAGS = 4  # the forest's F <= 256


def _check_masks(masks: torch.Tensor) -> int:
    if not isinstance(masks, torch.Tensor):
        raise ValueError("masks must be a GPU tensor")
    N.check_cuda(masks, "masks", torch.int64)
    if masks.dim() != 1:
        raise ValueError("masks must be a 1-D int64 tensor of feature masks")
    return masks.shape[0]


def _check_window(n: int, first: int, count: int, reach: int, what: str) -> None:
    """Samples first .. first+count-1, each reading ``reach`` draws past its own index."""
    if count < 1:
        raise ValueError(f"{what}: needs at least one sample (got {count})")
    if first < 0 or first + count + reach > n:
        raise ValueError(f"{what}: samples [{first}, {first + count}) read draws up to {first + count + reach - 1}, "
                         f"past the end of {n} masks")


def _check_out(t: torch.Tensor, name: str, dtype, shape, device) -> None:
    N.check_cuda(t, name, dtype)
    if tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError(f"{name} must be a {dtype} tensor of shape {tuple(shape)} on {device}")


def rf_words(lags: int) -> int:
    return (NF * lags + 63) // 64


def rf_rows(masks: torch.Tensor, lags: int = 1, first: int = 0, count: int | None = None,
            out: tuple[torch.Tensor, torch.Tensor] | None = None) -> tuple[torch.Tensor, torch.Tensor, int]:
    """(X int64 [S, W], Y int64 [S], F) on the device.  Sample ``s`` of ``[0, S)`` has the draws
    ``first+s .. first+s+lags-1`` as its input window (feature ``k*62 + j`` = bit ``j`` of draw ``first+s+k``,
    packed as ``forest.pack_bits``) and draw ``first+s+lags`` as its target.  ``count=None``: every sample from
    ``first`` on.  ``out``: (X, Y) to fill."""
    n = _check_masks(masks)
    lags, first = int(lags), int(first)
    if not 1 <= lags <= MAX_LAGS:
        raise ValueError(f"lags must be in 1..{MAX_LAGS} (the forest takes at most 256 features), got {lags}")
    S = n - lags - first if count is None else int(count)
    _check_window(n, first, S, lags, "rf_rows")
    W = rf_words(lags)
    if out is None:
        X = torch.empty(S, W, dtype=torch.int64, device=masks.device)
        Y = torch.empty(S, dtype=torch.int64, device=masks.device)
    else:
        X, Y = out
        _check_out(X, "X", torch.int64, (S, W), masks.device)
        _check_out(Y, "Y", torch.int64, (S,), masks.device)
    N.call("em_rf_lag_rows", masks.data_ptr(), n, first, S, lags, X.data_ptr(), W, Y.data_ptr(),
           N.stream_handle(masks.device))
    return X, Y, NF * lags


def bit_counts(masks: torch.Tensor, a: int = 0, b: int | None = None) -> np.ndarray:
    """int64 [64] on the host: ``counts[j]`` = number of masks in ``[a, b)`` with bit ``j`` set."""
    n = _check_masks(masks)
    a, b = int(a), n if b is None else int(b)
    if not 0 <= a <= b <= n:
        raise ValueError(f"bit_counts: range [{a}, {b}) outside the {n} masks")
    nb = N.query("em_mask_bit_count_blocks", b - a)
    part = torch.empty(max(nb, 1), 64, dtype=torch.int64, device=masks.device)
    counts = torch.empty(64, dtype=torch.int64, device=masks.device)
    N.call("em_mask_bit_counts", masks.data_ptr(), n, a, b, part.data_ptr(), counts.data_ptr(),
           N.stream_handle(masks.device))
    return counts.cpu().numpy()


def gbdt_draw_inputs(masks: torch.Tensor, first: int, count: int, varied: int,
                     out: tuple[torch.Tensor, torch.Tensor | None] | None = None, targets: bool = True
                     ) -> tuple[torch.Tensor, torch.Tensor | None]:
    """(bins uint8 [S, 62], Y float32 [S, 62]) on the device: ``bins[s, f]`` = bit ``f`` of draw ``first+s`` where
    bit ``f`` of ``varied`` is set (a column with the one cut 0.5), else 0 (a constant column: no cut, bin 0);
    ``Y[s, t]`` = bit ``t`` of draw ``first+s+1``.  ``out``: (bins, Y) to fill.  ``targets=False``: the bins alone
    (Y is None, and the last sample may be the last draw)."""
    n = _check_masks(masks)
    first, S = int(first), int(count)
    _check_window(n, first, S, 1 if targets else 0, "gbdt_draw_inputs")
    bins, Y = out if out is not None else (None, None)
    if bins is None:
        bins = torch.empty(S, NF, dtype=torch.uint8, device=masks.device)
    else:
        _check_out(bins, "bins", torch.uint8, (S, NF), masks.device)
    if not targets:
        Y = None
    elif Y is None:
        Y = torch.empty(S, NF, dtype=torch.float32, device=masks.device)
    else:
        _check_out(Y, "Y", torch.float32, (S, NF), masks.device)
    N.call("em_gbdt_draw_inputs", masks.data_ptr(), n, first, S, int(varied) & ((1 << NF) - 1), bins.data_ptr(),
           Y.data_ptr() if Y is not None else None, N.stream_handle(masks.device))
    return bins, Y


def varied_mask(counts, rows: int) -> int:
    """Bit ``f`` set iff column ``f`` takes both values over the ``rows`` counted masks."""
    return sum(1 << f for f in range(NF) if 0 < int(counts[f]) < int(rows))
