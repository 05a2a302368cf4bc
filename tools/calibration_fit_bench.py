#!/usr/bin/env python3
"""Scaling kernel benchmark (csrc/calibration_fit.hip) against a device-to-device copy, 1xMI355X.

    python tools/calibration_fit_bench.py [--rows 1048576,16777216] [--reps 20] [--out profiles/r18/calibration_fit_bench.jsonl]

On the SAME fp32 logits [rows, 64] (256 B per row, one row per lane), per row count:
  * em_scaling_stats under both heads (reads 256 + 8 B per row) and em_scaling_apply out of place (reads and writes
    256 B per row),
  * a device-to-device copy of the logits, the yardstick (reads and writes 256 B per row),
each as the median over --reps device-event timings of single launches, alternated, after warm launches of each;
  * the same statistics written as PyTorch ops (in chunks of 2^20 rows, so the temporaries fit), timed the same way
    over --torch-reps launches,
  * one full ``fit_device`` per head (wall clock: it reads a [blocks, 2, 6] tensor back after every pass).
Prints one JSON line per row count (and appends it to --out) with the times, the bytes per second and the share of
the copy's rate.  There is no CPU path: without a GPU this fails.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TORCH_CHUNK = 1 << 20


def torch_stats(z: torch.Tensor, masks: torch.Tensor, loss: str, a, b) -> torch.Tensor:
    """The six statistics per group as PyTorch ops: fp32 [2, 6] on the device (fp32 sums in torch's own order)."""
    out = torch.zeros(2, 6, dtype=torch.float32, device=z.device)
    shifts = torch.arange(62, device=z.device)
    for c0 in range(0, z.shape[0], TORCH_CHUNK):
        zc = z[c0:c0 + TORCH_CHUNK, :62]
        y = ((masks[c0 + 1:c0 + 1 + zc.shape[0], None] >> shifts) & 1).float()
        for g, sl in enumerate((slice(0, 50), slice(50, 62))):
            zg, yg = zc[:, sl], y[:, sl]
            u = a[g] * zg + b[g]
            if loss == "softmax":
                q = torch.softmax(u, 1)
                zy = (yg * zg).sum(1) / yg.sum(1).clamp(min=1.0)
                ez = (q * zg).sum(1)
                out[g, 0] += (torch.logsumexp(u, 1) - a[g] * zy).sum()
                out[g, 1] += (ez - zy).sum()
                out[g, 3] += (q * (zg - ez[:, None]) ** 2).sum()
            else:
                sg = torch.sigmoid(u)
                w = sg * (1.0 - sg)
                out[g, 0] += (torch.nn.functional.softplus(u) - yg * u).sum()
                out[g, 1] += ((sg - yg) * zg).sum()
                out[g, 2] += (sg - yg).sum()
                out[g, 3] += (w * zg * zg).sum()
                out[g, 4] += (w * zg).sum()
                out[g, 5] += w.sum()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1048576,16777216")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "calibration_fit_bench measures on the GPU"
    from euromillioner_amd.data.device_gen import generate_masks
    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.ops import calibration_fit as CF
    from euromillioner_amd.ops import fused_mlp as FM

    dev = torch.device("cuda")
    stream = N.stream_handle(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    ok = True
    for B in [int(r) for r in a.rows.split(",")]:
        masks = generate_masks(B + 2, seed=0, planted=0.8, device=dev)
        logits = torch.empty(B, 64, dtype=torch.float32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        shifts = torch.arange(62, device=dev)
        for c0 in range(0, B, TORCH_CHUNK):  # N(0, 2^2) plus 3 on the drawn outputs: logits worth fitting
            chunk = logits[c0:c0 + TORCH_CHUNK]
            chunk.normal_(0.0, 2.0, generator=gen)
            chunk[:, :62] += 3.0 * ((masks[c0 + 1:c0 + 1 + chunk.shape[0], None] >> shifts) & 1).float()
        other = torch.empty_like(logits)
        parts = torch.empty(CF.scaling_blocks(B), 2, 6, dtype=torch.float32, device=dev)
        av, bv = (ctypes.c_float * 2)(1.25, 0.75), (ctypes.c_float * 2)(0.0, 0.0)
        ap_, bp_ = ctypes.cast(av, ctypes.c_void_p), ctypes.cast(bv, ctypes.c_void_p)

        def stats(kind):  # raw launches: nothing but the kernel between the two events
            N.call("em_scaling_stats", logits.data_ptr(), 64, masks.data_ptr(), None, B, 0, kind, ap_, bp_,
                   parts.data_ptr(), stream)

        runs = {"stats_softmax": lambda: stats(FM.LOSS_KINDS["softmax"]), "stats_bce": lambda: stats(FM.LOSS_KINDS["bce"]),
                "apply": lambda: N.call("em_scaling_apply", logits.data_ptr(), 64, B, ap_, bp_, other.data_ptr(), 64, stream),
                "copy": lambda: other.copy_(logits)}
        for fn in runs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.reps):  # alternated: drift of the clocks lands on all alike
            for k, fn in runs.items():
                times[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        nbytes = {"stats_softmax": 264 * B, "stats_bce": 264 * B, "apply": 512 * B, "copy": 512 * B}
        rate = {k: nbytes[k] / med[k] for k in runs}
        res = {"metric": "em_scaling_stats / em_scaling_apply vs a device-to-device copy of the same logits", "rows": B,
               "reps": a.reps, "bytes_per_row": nbytes["stats_bce"] // B,
               **{k + "_s": med[k] for k in runs}, **{k + "_min_max_s": [min(v), max(v)] for k, v in times.items()},
               "bytes_per_s": rate, "share_of_copy_rate": {k: rate[k] / rate["copy"] for k in runs if k != "copy"}}
        # the same statistics as PyTorch ops, and the agreement of the two
        at, bt = (1.25, 0.75), (0.0, 0.0)
        for loss in ("softmax", "bce"):
            ref = torch_stats(logits, masks, loss, at, bt)
            t = [timed(lambda: torch_stats(logits, masks, loss, at, bt)) for _ in range(a.torch_reps)]
            res[f"torch_stats_{loss}_s"] = float(np.median(t))
            res[f"torch_over_kernel_{loss}"] = res[f"torch_stats_{loss}_s"] / med[f"stats_{loss}"]
            got = CF.sum_scaling(CF.scaling_stats(logits, masks, B, loss, at, bt, out=parts))
            want = ref.double().cpu().numpy()
            rel = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))
            res[f"max_rel_diff_to_torch_{loss}"] = rel
            ok = ok and rel < 1e-3  # (torch sums hundreds of millions of fp32 terms in fp32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit = CF.fit_device(logits, masks, B, loss)
            res[f"fit_{loss}"] = {"wall_s": time.perf_counter() - t0, "passes": fit["passes"],
                                  "iterations": fit["iterations"], "converged": fit["converged"],
                                  "a": [float(v) for v in fit["a"]], "b": [float(v) for v in fit["b"]]}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")
        del logits, other, masks, parts
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
