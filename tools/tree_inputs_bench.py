#!/usr/bin/env python3
"""Tree-model inputs: the host featurisation against the device kernels (csrc/tree_inputs.hip), 1xMI355X.

    python tools/tree_inputs_bench.py [--draws 700000] [--lags 1,2] [--windows 7] [--launches 50] [--repeat 3]
                                      [--out profiles/r15/tree_inputs_bench.jsonl]

For every lag count, on the same generated draws:

* forest, host: ``models.forest.draw_features`` on the draw rows plus the upload of X and Y, host clock around a
  call that ends in a device synchronise (the first call is dropped, the median of ``--repeat`` is reported);
* forest, device: ``em_rf_lag_rows`` on the masks, device events around windows of ``--launches`` back-to-back
  launches into preallocated buffers after a warm-up; per-launch median and min / max over the windows;
* GBDT (lag 1 only, the task has no lag windows), host: ``multi_hot`` + ``make_cuts`` + ``apply_bins`` plus the uint8
  and float32 uploads, as ``GBDT.fit`` / ``gbdt_hip.fit`` do them;
* GBDT, device: ``em_mask_bit_counts`` (with the download of the 64 counts, host clock) and
  ``em_gbdt_draw_inputs`` (device events, as above), with the bytes each launch writes over its time.

The outputs of both sides are compared before anything is timed.  One JSON line per lag count, printed and
appended to ``--out``.  These are records, not pass criteria."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=700_000)
    ap.add_argument("--lags", default="1,2")
    ap.add_argument("--planted", type=float, default=0.9)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3, help="timed host featurisations (one more is dropped)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from euromillioner_amd.data.draws import mask_bits, multi_hot
    from euromillioner_amd.data.synthetic import generate_draws
    from euromillioner_amd.models.forest import draw_features
    from euromillioner_amd.models.gbdt import apply_bins, cuts_from_bit_counts, make_cuts
    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.ops import tree_inputs as TI

    if not torch.cuda.is_available():
        raise SystemExit("tree_inputs_bench needs a GPU: a timing taken anywhere else says nothing about it")
    dev = torch.device("cuda")
    nums, _ = generate_draws(a.draws, seed=0, planted=a.planted, native=True)
    masks = torch.from_numpy(mask_bits(nums).view(np.int64)).to(dev)
    st = N.stream_handle(dev)

    def host_median(fn):
        t = []
        for _ in range(1 + a.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return {"median_s": statistics.median(t[1:]), "min_s": min(t[1:]), "max_s": max(t[1:]), "first_call_s": t[0]}

    def device_windows(fn):
        for _ in range(5):  # warm-up: code objects, clocks
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.launches)
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    rows = []
    for lags in [int(v) for v in a.lags.split(",") if v]:
        S = a.draws - lags
        W = TI.rf_words(lags)
        keep = {}

        def rf_host():
            X, Y, _ = draw_features(nums, lags)
            keep["X"] = torch.from_numpy(np.ascontiguousarray(X).view(np.int64)).to(dev)
            keep["Y"] = torch.from_numpy(np.ascontiguousarray(Y).view(np.int64)).to(dev)

        Xd = torch.empty(S, W, dtype=torch.int64, device=dev)
        Yd = torch.empty(S, dtype=torch.int64, device=dev)

        def rf_device():
            N.call("em_rf_lag_rows", masks.data_ptr(), a.draws, 0, S, lags, Xd.data_ptr(), W, Yd.data_ptr(), st)

        rf_h = host_median(rf_host)
        rf_d = device_windows(rf_device)
        if not (torch.equal(Xd, keep["X"].reshape(S, W)) and torch.equal(Yd, keep["Y"])):
            raise SystemExit(f"lags {lags}: em_rf_lag_rows differs from draw_features")
        rf_bytes = 8 * S * (W + 1)
        row = {"metric": "tree-model inputs from draw masks", "draws": a.draws, "lags": lags, "samples": S,
               "windows": a.windows, "launches_per_window": a.launches, "host_repeats": a.repeat,
               "rf_host_draw_features_upload": rf_h, "em_rf_lag_rows": rf_d, "em_rf_lag_rows_bytes_written": rf_bytes,
               "em_rf_lag_rows_gb_per_s": rf_bytes / (rf_d["median_ms"] * 1e-3) / 1e9,
               "rf_host_over_device": rf_h["median_s"] / (rf_d["median_ms"] * 1e-3)}
        if lags == 1:
            n = a.draws - 1

            def gbdt_host():
                X = multi_hot(nums[:-1]).astype(np.float64)
                Y = multi_hot(nums[1:]).astype(np.float64)
                cuts = make_cuts(X, 256)
                bins = apply_bins(X, cuts)
                keep["cuts"] = cuts
                keep["bins"] = torch.from_numpy(np.ascontiguousarray(bins, dtype=np.uint8)).to(dev)
                keep["GY"] = torch.from_numpy(np.ascontiguousarray(Y, dtype=np.float32)).to(dev)

            bins_d = torch.empty(n, 62, dtype=torch.uint8, device=dev)
            gy_d = torch.empty(n, 62, dtype=torch.float32, device=dev)
            counts = TI.bit_counts(masks, 0, n)
            varied = TI.varied_mask(counts, n)

            def gbdt_device():
                N.call("em_gbdt_draw_inputs", masks.data_ptr(), a.draws, 0, n, varied, bins_d.data_ptr(),
                       gy_d.data_ptr(), st)

            g_h = host_median(gbdt_host)
            g_c = host_median(lambda: TI.bit_counts(masks, 0, n))
            g_d = device_windows(gbdt_device)
            same_cuts = all(np.array_equal(x, y) for x, y in zip(keep["cuts"], cuts_from_bit_counts(counts[:62], n)))
            if not (same_cuts and torch.equal(bins_d, keep["bins"]) and torch.equal(gy_d, keep["GY"])):
                raise SystemExit("em_gbdt_draw_inputs / bit_counts differ from multi_hot + make_cuts + apply_bins")
            g_bytes = n * 62 * 5
            row.update({"gbdt_host_multi_hot_cuts_bins_upload": g_h, "bit_counts_with_download": g_c,
                        "em_gbdt_draw_inputs": g_d, "em_gbdt_draw_inputs_bytes_written": g_bytes,
                        "em_gbdt_draw_inputs_gb_per_s": g_bytes / (g_d["median_ms"] * 1e-3) / 1e9,
                        "gbdt_host_over_device": g_h["median_s"] / (g_c["median_s"] + g_d["median_ms"] * 1e-3)})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a", encoding="utf-8") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
