#!/usr/bin/env python3
"""Calibration kernel benchmark (csrc/calibration.hip) against the draw-metric kernel, 1xMI355X.

    python tools/calibration_bench.py [--rows 4194304] [--reps 20] [--out profiles/r17/calibration_bench.jsonl]

On the SAME fp32 logits [rows, 64] (256 B per row, one row per lane in all three), per head kind:
  * em_draw_calibration without and with the per-element ``bins`` output,
  * em_draw_metrics, the yardstick: the existing kernel that streams the same bytes,
each as the median over --reps device-event timings of single launches, alternated, after warm launches of each.
Prints one JSON line (and appends it to --out) with the times, the ratios to em_draw_metrics and the share of the
HBM stream rate.  There is no CPU path: without a GPU this fails.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "calibration_bench measures on the GPU"
    from euromillioner_amd import calibration as CAL
    from euromillioner_amd.data.device_gen import generate_masks
    from euromillioner_amd.models.mlp import FusedSmallMLP
    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.ops import calibration as OC
    from euromillioner_amd.ops import fused_mlp as FM

    dev = torch.device("cuda")
    B = a.rows
    masks = generate_masks(B + 2, seed=0, planted=0.8, device=dev)
    model = FusedSmallMLP(dev, lr=3e-3)
    for s in range(20):
        model.step(masks, min(B, 1 << 16), offset=(s * (1 << 16)) % max(B - (1 << 16), 1))
    logits = model.logits(masks, B)
    torch.cuda.synchronize()
    nb = OC.calibration_blocks(B)
    out = {"counts": torch.empty(nb, 2, 16, dtype=torch.int32, device=dev),
           "hits": torch.empty(nb, 2, 16, dtype=torch.int32, device=dev),
           "sum_q": torch.empty(nb, 2, 16, dtype=torch.float32, device=dev),
           "brier": torch.empty(nb, 2, dtype=torch.float32, device=dev)}
    out_bins = dict(out, bins=torch.empty(B, 64, dtype=torch.uint8, device=dev))
    part8 = torch.empty(nb, 8, dtype=torch.float32, device=dev)
    stream = N.stream_handle(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    res = {"metric": "calibration totals (em_draw_calibration) vs em_draw_metrics on the same logits", "rows": B,
           "reps": a.reps, "bytes_per_row": 256 + 8, "heads": {}}
    for loss in ("softmax", "bce"):
        OC.draw_calibration(logits, masks, B, loss, want_bins=True, out=out_bins)  # (the checked path, once)
        ex = CAL.edges_x(CAL.DEFAULT_EDGES, loss)
        ebuf = (ctypes.c_float * len(ex))(*[float(v) for v in ex])
        kind = FM.LOSS_KINDS[loss]

        def cal(bins, kind=kind, ebuf=ebuf):  # raw launches: nothing but the kernel between the two events
            N.call("em_draw_calibration", logits.data_ptr(), 64, masks.data_ptr(), None, B, 0, kind,
                   ctypes.cast(ebuf, ctypes.c_void_p), len(ebuf), out["counts"].data_ptr(), out["hits"].data_ptr(),
                   out["sum_q"].data_ptr(), out["brier"].data_ptr(), bins, stream)

        runs = {"calibration": lambda: cal(None), "calibration_bins": lambda: cal(out_bins["bins"].data_ptr()),
                "draw_metrics": lambda kind=kind: N.call("em_draw_metrics", logits.data_ptr(), 64, masks.data_ptr(), None,
                                                         B, 0, kind, part8.data_ptr(), stream)}
        for fn in runs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.reps):  # alternated: drift of the clocks lands on all three alike
            for k, fn in runs.items():
                times[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        tot = OC.sum_calibration(out)
        head = {k + "_s": med[k] for k in runs}
        head.update({k + "_min_max_s": [min(v), max(v)] for k, v in times.items()})
        head["ratio_calibration_over_draw_metrics"] = med["calibration"] / med["draw_metrics"]
        head["ratio_calibration_bins_over_draw_metrics"] = med["calibration_bins"] / med["draw_metrics"]
        head["share_of_hbm_stream"] = {k: (B * (256 + 8) + (B * 64 if k == "calibration_bins" else 0)) / med[k] / HBM_BYTES_PER_S
                                       for k in runs}
        head["rows_per_s_calibration"] = B / med["calibration"]
        head["invariants_ok"] = bool(tot["counts"].sum(1).tolist() == [50 * B, 12 * B]
                                     and tot["hits"].sum(1).tolist() == [5 * B, 2 * B])
        head["ece_main"] = CAL.report(tot, B, loss)["main"]["ece"]
        res["heads"][loss] = head
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0 if all(h["invariants_ok"] for h in res["heads"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
