"""Python face of ``csrc/tickets.hip``: tickets sampled from logits on the GPU and their prize tiers.

The specification is :mod:`euromillioner_amd.tickets` (numpy); the kernel consumes the logits that a model's
``logits()`` already produced, so the trained kernels are untouched."""
from __future__ import annotations

import numpy as np
import torch

from .. import tickets as TK
from . import _native as N
from .fused_mlp import _check_draws

M64 = (1 << 64) - 1


def ticket_blocks(B: int, n_tickets: int) -> int:
    """Rows of the partials that :func:`draw_tickets` returns (one per block of whole rows)."""
    return int(N.query("em_ticket_blocks", int(B), int(n_tickets)))


def draw_tickets(logits: torch.Tensor, B: int, n_tickets: int, temperature: float = 1.0, seed: int = 0,
                 masks: torch.Tensor | None = None, offset: int = 0, sidx: torch.Tensor | None = None,
                 row_base: int = 0, want_tickets: bool = True, want_keys: bool = False) -> dict:
    """``n_tickets`` tickets for each of the first B rows of ``logits`` [>= B, 64] (fp32).

    The RNG row id of row s is ``row_base + (sidx[s] if sidx is not None else offset + s)``; with ``masks``
    every ticket is scored against draw ``masks[that index + 1]`` (as ``draw_metrics``).  Returns
    ``tickets`` int64 [B, N] (bit pattern = uint64 mask; ``want_tickets``), ``keys`` fp32 [B, N, 64]
    (``want_keys``; columns 62-63 are 0) and, with ``masks``, ``partials`` int32 [blocks, 32]: columns 0-17 the
    tickets per hit cell ``m * 3 + s``, columns 18-31 the rows by best rank 1..14."""
    n_tickets, B = int(n_tickets), int(B)
    TK.check_n_t(n_tickets, float(temperature))
    N.check_cuda(logits, "logits", torch.float32, contiguous=False)
    if logits.dim() != 2 or logits.shape[1] < 64 or logits.stride(1) != 1 or logits.stride(0) % 4 or logits.shape[0] < B:
        raise ValueError("logits must be [>= B, >= 64] fp32 rows with a row stride that is a multiple of 4")
    if B < 0 or row_base < 0:
        raise ValueError("B and row_base must be >= 0")
    if masks is not None:
        _check_draws(masks, sidx, B, offset)
    else:
        if B >= 2**31 - 1:
            raise ValueError("at most 2^31-2 samples per call")
        if sidx is not None:
            N.check_cuda(sidx, "sample_idx", torch.int32)
            if sidx.numel() < B:
                raise ValueError("sample_idx shorter than B")
        elif offset < 0:
            raise ValueError("offset must be >= 0")
    dev = logits.device
    out: dict = {}
    tickets = torch.empty(B, n_tickets, dtype=torch.int64, device=dev) if want_tickets else None
    keys = torch.empty(B, n_tickets, 64, dtype=torch.float32, device=dev) if want_keys else None
    part = None
    if masks is not None:
        part = torch.zeros(max(ticket_blocks(B, n_tickets), 1), 32, dtype=torch.int32, device=dev)
    if B > 0:
        N.call("em_draw_tickets", logits.data_ptr(), logits.stride(0), N.ptr(masks), N.ptr(sidx), B, int(offset),
               int(row_base), n_tickets, float(temperature), int(seed) & M64, N.ptr(tickets), N.ptr(keys), N.ptr(part),
               N.stream_handle(dev))
    if tickets is not None:
        out["tickets"] = tickets
    if keys is not None:
        out["keys"] = keys
    if part is not None:
        out["partials"] = part if B > 0 else part[:0]
    return out


def sum_partials(part: torch.Tensor) -> tuple[np.ndarray, np.ndarray]:
    """partials [blocks, 32] -> (hist [6, 3], best [14]) summed in int64."""
    tot = part.to(torch.int64).sum(0).cpu().numpy()
    return tot[:18].reshape(6, 3).copy(), tot[18:32].copy()


def backtest_result(hist: np.ndarray, best: np.ndarray, rows: int, n_tickets: int) -> dict:
    """The common result of every back-test (GPU or numpy): counts next to their uniform-play expectation."""
    u = TK.uniform_expectation(n_tickets)
    return {"hist": np.asarray(hist, dtype=np.int64), "best": np.asarray(best, dtype=np.int64), "rows": int(rows),
            "tickets": int(rows) * int(n_tickets),
            "uniform": {"hist": u["hist"] * rows * n_tickets, "tiers": u["rank"] * rows * n_tickets,
                        "best": u["best"] * rows}}


def backtest_model(model, masks: torch.Tensor, B: int, n_tickets: int, temperature: float = 1.0, seed: int = 0,
                   offset: int = 0, sidx: torch.Tensor | None = None, chunk: int = 1 << 20,
                   target_masks: torch.Tensor | None = None) -> dict:
    """Play ``n_tickets`` sampled tickets on each of B samples and count prize tiers: ``model.logits`` then
    :func:`draw_tickets` in chunks (the logits of one chunk are the only intermediate).  ``target_masks``:
    the masks as the scoring sees them when the model's target is not ``masks[i + 1]`` (lag windows).
    Returns ``{"hist", "best", "rows", "tickets", "uniform"}``; the integers do not depend on ``chunk``."""
    if getattr(model, "group", None) is not None:
        raise ValueError("backtest is single-process (no process group)")
    TK.check_n_t(n_tickets, float(temperature))
    if chunk < 1:
        raise ValueError("chunk >= 1")
    tm = masks if target_masks is None else target_masks
    _check_draws(tm, sidx, B, offset)
    hist, best = np.zeros((6, 3), dtype=np.int64), np.zeros(14, dtype=np.int64)
    done = 0
    while done < B:
        b = min(chunk, B - done)
        o = offset + done if sidx is None else 0
        si = None if sidx is None else sidx[done:done + b]
        lg = model.logits(masks, b, offset=o, sidx=si)
        r = draw_tickets(lg, b, n_tickets, temperature, seed, masks=tm, offset=o, sidx=si, want_tickets=False)
        h, bt = sum_partials(r["partials"])
        hist += h
        best += bt
        done += b
    return backtest_result(hist, best, B, n_tickets)
